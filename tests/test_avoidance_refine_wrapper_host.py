"""conjunction.avoidance_refine without a device: argument checks and their messages, the empty list (no library call), the refusal of
more than one device, and AvoidanceRefineResult."""
import numpy as np
import pytest


def plan(S=3, K=5):
    return dict(Y=np.ones((S, 7, K)), U=np.zeros((S, 3, K)), units=np.ones((S, 2)), span=np.array([[0.0, 1.0]] * S), consts=np.ones((S, 8)))


GRID = dict(M=9, T0=0.0, T1=1.0)
PAIRS = np.array([[0.0, 1.0, 10.0, 0.5], [1.0, 2.0, 10.0, 0.6]])


def test_argument_checks_and_messages():
    from mpconstellation_amd import avoidance_refine
    S, K, D, Kc = 3, 5, 2, 4
    cat = (np.ones((D, 7, Kc)), np.ones((D, 2)), np.array([[0.0, 1.0]] * D))
    P = np.zeros((S, K, 6, 6))
    good = dict(pairs=PAIRS, target=100.0, **plan(S, K), **GRID)
    for bad, text in ((dict(pairs=np.zeros((1, 3))), "pairs"), (dict(target=0.0), "target"), (dict(target=np.nan), "target"), (dict(tol=0.0), "tol"),
                      (dict(max_iter=0), "max_iter"), (dict(who="both"), "who"), (dict(who=np.array([0, 2])), "who"), (dict(cat=cat, who="j"), "catalogue"),
                      (dict(Y=np.ones((S, 6, K))), "Y"), (dict(U=np.zeros((S, 3, K + 1))), "U"), (dict(consts=np.ones((S, 7))), "consts"),
                      (dict(ns=np.array([5])), "ns"), (dict(cat=cat, P=P), "cat_P"), (dict(u_max=0.0), "u_max"), (dict(max_step=0.0), "max_step"),
                      (dict(mu=0.0), "mu"),
                      # the refinement's own
                      (dict(rounds=-1), "rounds"), (dict(rounds=1.5), "rounds"), (dict(rounds=np.array([1, 2])), "rounds"), (dict(M=1), "M"),
                      (dict(M=4.5), "M"), (dict(T1=0.0), "T0 < T1"), (dict(T0=np.nan), "T0 < T1"), (dict(prop_max_step=0.0), "prop_max_step"),
                      (dict(prop_max_step=-1e-3), "prop_max_step")):
        with pytest.raises(ValueError, match=text):
            avoidance_refine(**{**good, **bad})


def test_more_than_one_device_is_rejected():
    from mpconstellation_amd import avoidance_refine
    with pytest.raises(ValueError, match="one device .every round needs every mover's new trajectory."):
        avoidance_refine(PAIRS, 100.0, **plan(), **GRID, devices=[0, 1])
    with pytest.raises(ValueError, match="one device"):                    # (refused before the empty list is answered)
        avoidance_refine(np.zeros((0, 4)), 100.0, **plan(), **GRID, devices=[0, 1])


def test_empty_list_returns_zeros_without_a_library_call():
    from mpconstellation_amd import avoidance_refine, AvoidanceRefineResult, AvoidanceJointResult
    S, K = 3, 5
    p = plan(S, K)
    p["Y"] = np.arange(S * 7 * K, dtype=np.float64).reshape(S, 7, K) + 1.0
    res = avoidance_refine(np.zeros((0, 4)), 100.0, **p, **GRID, rounds=2, u_max=2.0, return_rows=True, return_terminal=True, return_rhs=True, devices=[0])
    assert isinstance(res, AvoidanceRefineResult) and isinstance(res, AvoidanceJointResult)
    assert res.du.shape == (S, 3, K) and not res.du.any() and not res.sat_out.any() and res.status.tolist() == [0] * S
    assert res.rows.shape == (0, 3, K) and res.tsens.shape == (S, 6, 3, K) and not res.tsens.any() and res.row_out.shape == (0, 5)
    assert np.array_equal(res.Y_flown, p["Y"]) and res.Y_flown is not p["Y"] and res.pairs_flown.shape == (0, 4)
    assert res.d0_history.shape == (4, 0) and res.tca_history.shape == (4, 0) and res.terminal_history.shape == (4, S) and not res.terminal_history.any()
    assert res.rounds_done.tolist() == [-1] * S and res.rounds_done.dtype == np.int32 and res.rhs_rows.shape == (0,) and res.rhs_term.shape == (S, 6)
    bare = avoidance_refine(np.zeros((0, 4)), 100.0, **p, **GRID, rounds=0)
    assert bare.rows is None and bare.tsens is None and bare.rhs_rows is None and bare.rhs_term is None and bare.d0_history.shape == (2, 0)
    U = np.arange(S * 3 * K, dtype=np.float64).reshape(S, 3, K)
    assert np.array_equal(res.apply(U), U) and res.apply(U) is not U and "passes=4" in repr(res)


def test_apply_behaves_as_the_joint_result():
    from mpconstellation_amd import AvoidanceRefineResult, _ffi
    S, K = 2, 4
    du = np.arange(S * 3 * K, dtype=np.float64).reshape(S, 3, K)
    mk = lambda status: AvoidanceRefineResult((PAIRS[:1], np.zeros(1, dtype=np.int32), du, np.zeros((S, _ffi.NAJ)), np.zeros((1, _ffi.NAR)), None, None,
                                               np.asarray(status, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=bool)),
                                              np.ones((S, 7, K)), PAIRS[:1], np.zeros((2, 1)), np.zeros((2, 1)), np.zeros((2, S)),
                                              np.zeros(S, dtype=np.int32), None, None)
    U = np.ones((S, 3, K))
    assert np.array_equal(mk([0, 0]).apply(U), U + du) and mk([0, 0]).lam.shape == (1,)
    with pytest.raises(ValueError, match="satellite 1 has no manoeuvre: solver hit max_iter"):
        mk([0, 5]).apply(U)


def test_constellation_mpc_checks_the_model():
    from mpconstellation_amd import ConstellationMPC
    assert "model" in ConstellationMPC.avoidance_refine.__code__.co_varnames and "install" in ConstellationMPC.avoidance_refine.__code__.co_varnames
