"""conjunction.avoidance_joint without a device: argument checks and their messages, the forms of `who`, `coupled`, the empty list
(no library call) and AvoidanceJointResult.apply."""
import numpy as np
import pytest


def plan(S=3, K=5):
    return dict(Y=np.ones((S, 7, K)), U=np.zeros((S, 3, K)), units=np.ones((S, 2)), span=np.array([[0.0, 1.0]] * S), consts=np.ones((S, 8)))


def test_argument_checks_and_messages():
    from mpconstellation_amd import avoidance_joint
    S, K, D, Kc = 3, 5, 2, 4
    pairs = np.array([[0.0, 1.0, 10.0, 0.5], [1.0, 2.0, 10.0, 0.6]])
    cat = (np.ones((D, 7, Kc)), np.ones((D, 2)), np.array([[0.0, 1.0]] * D))
    P, cP = np.zeros((S, K, 6, 6)), np.zeros((D, Kc, 6, 6))
    good = dict(pairs=pairs, target=100.0, **plan(S, K))
    for bad, text in ((dict(pairs=np.zeros((1, 3))), "pairs"), (dict(target=0.0), "target"), (dict(target=np.inf), "target"), (dict(target=np.nan), "target"),
                      (dict(tol=0.0), "tol"), (dict(tol=np.inf), "tol"), (dict(max_iter=0), "max_iter"), (dict(max_iter=2.5), "max_iter"),
                      (dict(who="both"), "who"), (dict(who="k"), "who"), (dict(who=np.array([0, 1, 0])), "who"), (dict(who=np.array([0, 2])), "who"),
                      (dict(who=np.array([[0, 1]])), "who"), (dict(cat=cat, who="j"), "catalogue"), (dict(cat=cat, who=np.array([0, 1])), "catalogue"),
                      (dict(Y=np.ones((S, 6, K))), "Y"), (dict(U=np.zeros((S, 3, K + 1))), "U"), (dict(consts=np.ones((S, 7))), "consts"),
                      (dict(ns=np.array([5])), "ns"), (dict(P=np.zeros((S, K, 6, 5))), "P"), (dict(cat=cat, P=P), "cat_P"), (dict(cat=cat + (cP,)), "cat_P"),
                      (dict(cat=cat[:2]), "cat"), (dict(u_max=np.ones(S + 1)), "u_max"), (dict(u_max=np.ones((S, 1))), "u_max"), (dict(u_max=0.0), "u_max"),
                      (dict(u_max=np.array([1.0, -1.0, 1.0])), "u_max"), (dict(u_max=np.nan), "u_max"), (dict(max_step=0.0), "max_step"), (dict(mu=0.0), "mu")):
        with pytest.raises(ValueError, match=text):
            avoidance_joint(**{**good, **bad})


def test_empty_list_returns_zeros_without_a_library_call():
    from mpconstellation_amd import avoidance_joint, AvoidanceJointResult, conjunction
    S, K = 3, 5
    res = avoidance_joint(np.zeros((0, 4)), 100.0, **plan(S, K), u_max=2.0, return_rows=True, return_terminal=True)
    assert isinstance(res, AvoidanceJointResult) and res.du.shape == (S, 3, K) and not res.du.any() and not res.sat_out.any()
    assert res.status.tolist() == [0] * S and res.rows.shape == (0, 3, K) and res.tsens.shape == (S, 6, 3, K) and not res.tsens.any()
    assert res.row_out.shape == (0, 5) and res.coupled.shape == (0,) and res.mover.shape == (0,) and res.d0.shape == (0,)
    assert conjunction.avoidance_joint(np.zeros((0, 4)), 100.0, **plan(S, K), who=np.zeros(0, dtype=int)).rows is None
    U = np.arange(S * 3 * K, dtype=np.float64).reshape(S, 3, K)
    assert np.array_equal(res.apply(U), U) and res.apply(U) is not U


def test_who_forms_and_coupled():
    from mpconstellation_amd.conjunction import _check_mover, _coupled
    assert _check_mover("i", 3, False).tolist() == [0, 0, 0] and _check_mover("j", 2, False).tolist() == [1, 1]
    m = _check_mover([0, 1, 1], 3, False)
    assert m.dtype == np.int32 and m.flags.c_contiguous and m.tolist() == [0, 1, 1]
    assert _check_mover(np.array([True, False]), 2, False).tolist() == [1, 0] and _check_mover("i", 2, True).tolist() == [0, 0]
    # pairs (0,1) (0,2) (1,2) (3,4): with i moving, the still object of (0,1) -- satellite 1 -- is moved by row (1,2); satellite 2 and 4 never move
    pairs = np.array([[0.0, 1.0, 5.0, 0.1], [0.0, 2.0, 5.0, 0.2], [1.0, 2.0, 5.0, 0.3], [3.0, 4.0, 5.0, 0.4]])
    assert _coupled(pairs, _check_mover("i", 4, False), False).tolist() == [True, False, False, False]
    assert _coupled(pairs, _check_mover("j", 4, False), False).tolist() == [False, False, True, False]
    assert _coupled(pairs, _check_mover([0, 1, 1, 1], 4, False), False).tolist() == [False, True, False, False]
    assert _coupled(pairs, _check_mover("i", 4, True), True).tolist() == [False] * 4             # a catalogue object is nobody's to move


def test_apply():
    from mpconstellation_amd import AvoidanceJointResult, _ffi
    S, K = 3, 4
    pairs = np.array([[0.0, 1.0, 5.0, 0.1], [2.0, 1.0, 5.0, 0.2]])
    du = np.arange(S * 3 * K, dtype=np.float64).reshape(S, 3, K)
    du[1] = 0.0
    mk = lambda status: AvoidanceJointResult(pairs, np.zeros(2, dtype=np.int32), du, np.zeros((S, _ffi.NAJ)), np.zeros((2, _ffi.NAR)), None, None,
                                             np.asarray(status, dtype=np.int32), np.zeros(2, dtype=np.int32), np.zeros(2, dtype=bool))
    U = np.ones((S, 3, K))
    U2 = mk([0, 0, 0]).apply(U)
    assert np.array_equal(U2, U + du) and (U == 1.0).all()
    with pytest.raises(ValueError, match="expected"):
        mk([0, 0, 0]).apply(np.ones((S, 3, K + 1)))
    with pytest.raises(ValueError, match="satellite 2 has no manoeuvre: constraint set empty"):
        mk([0, 0, 8]).apply(U)
    r = mk([0, 0, 0])
    assert r.cost.shape == (S,) and r.lam.shape == (2,) and "pairs=2" in repr(r)
