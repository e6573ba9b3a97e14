"""Screening against a catalogue without a device: the restated cross screen against the analytic truth, the wrappers' argument
checks, ConstellationMPC's hand-over of the catalogue and the windows, and combine / sort_pairs on pairs (i, j) with j < i."""
import numpy as np
import pytest

import conjunction_reference as R
import conjunction_cross_reference as X
from mpconstellation_amd import conjunction as cj
from test_conjunction_host import hand_made_mpc, true_minimum


def test_restated_cross_screen_against_analytic_truth():
    """20 satellites, 20 objects, node spacing h_n = 57 s, grid spacing h = 30 s: for the pairs (k, k) |restated minimum - true
    minimum| <= 2 B with B = 2 (h^4 + h_n^4) / 384 w^4 R, the bound of test_restatement_against_analytic_truth."""
    S, hn, h, n = 20, 57.0, 30.0, 101
    orb = R.random_orbits(2 * S, seed=7)
    T0, T1 = 0.0, hn * (n - 1)
    Y, units, span = R.trajectories(orb, n, (T0, T1))
    M = int(round((T1 - T0) / h)) + 1
    assert abs((T1 - T0) / (M - 1) - h) < 1e-9
    eph, status = R.ephemeris(Y, units, span, M, T0, T1)
    assert (status == 0).all() and not np.isnan(eph).any()
    ref = X.screen_against(eph[:S], eph[S:], T0, T1)
    assert ref.Q.shape == (S, S) and len(ref.pairs) == S * S and (ref.partner >= 0).all()
    w, Rr = R.orbit_rate(orb), orb["R"]
    worst = 0.0
    for k in range(S):
        truth = true_minimum(orb, k, S + k, T0, T1)
        B = 2.0 * (h ** 4 + hn ** 4) / 384.0 * max(w[k] ** 4 * Rr[k], w[S + k] ** 4 * Rr[S + k])
        err = abs(np.sqrt(ref.Q[k, k]) - truth)
        worst = max(worst, err / B)
        assert err <= 2.0 * B, (k, err, B)
    print(f"worst error / B = {worst:.3f}")
    # a row's result is the first minimum of its row of Q
    j = ref.partner[3]
    assert ref.dmin[3] == np.sqrt(ref.Q[3].min()) and ref.Q[3, j] == ref.Q[3].min() and ref.tca[3] == ref.T[3, j]


def test_wrapper_argument_checks(monkeypatch):
    """every bad argument is a ValueError before the library (which needs a device) is touched"""
    from mpconstellation_amd import _ffi

    def no_context(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_ffi, "context", no_context)
    monkeypatch.setattr(_ffi, "call", no_context)
    Y, units, span = np.zeros((2, 7, 5)), np.ones((2, 2)), np.array([[0.0, 1.0]] * 2)
    cY, cunits, cspan = np.zeros((3, 7, 9)), np.ones((3, 2)), np.array([[0.0, 1.0]] * 3)
    eph, cat = np.zeros((2, 6, 4)), np.zeros((3, 6, 4))
    traj = dict(Y=Y, units=units, span=span, cat_Y=cY, cat_units=cunits, cat_span=cspan, M=4, T0=0.0, T1=1.0)
    with pytest.raises(ValueError, match="common_clock"):
        cj.screen_against(eph=eph, cat_Y=cY, cat_units=cunits, cat_span=cspan, M=4, T0=0.0, T1=1.0)      # mixed
    with pytest.raises(ValueError, match="common_clock"):
        cj.screen_against(cat_eph=cat, Y=Y, units=units, span=span, M=4, T0=0.0, T1=1.0)                 # mixed, the other way
    bad_eph = [dict(cat_eph=None), dict(eph=None), dict(eph=np.zeros((2, 7, 4))), dict(cat_eph=np.zeros((3, 7, 4))), dict(cat_eph=np.zeros((3, 6, 5))),
               dict(cat_eph=np.zeros((0, 6, 4))), dict(eph=np.zeros((2, 6, 1)), cat_eph=np.zeros((3, 6, 1))), dict(M=5), dict(T0=None), dict(T1=0.0),
               dict(max_pairs=-1), dict(max_pairs=2.5), dict(threshold=np.nan)]
    for kw in bad_eph:
        args = dict(eph=eph, cat_eph=cat, T0=0.0, T1=1.0); args.update(kw)
        with pytest.raises(ValueError):
            cj.screen_against(**args)
    bad_traj = [dict(cat_Y=None), dict(Y=None), dict(M=None), dict(M=1), dict(cat_Y=np.zeros((3, 6, 9))), dict(cat_units=np.ones((2, 2))),
                dict(cat_units=None), dict(cat_span=np.ones((3, 3))), dict(cat_span=None), dict(cat_ns=[9, 9]), dict(ns=[5, 5, 5]),
                dict(units=np.ones((3, 2))), dict(T1=np.inf)]
    for kw in bad_traj:
        args = dict(traj); args.update(kw)
        with pytest.raises(ValueError):
            cj.screen_against(**args)
    with pytest.raises(ValueError, match="cat_units"):
        cj.screen_against(**{**traj, "cat_units": np.ones((3, 3))})
    with pytest.raises(ValueError):
        cj.screen_against(T0=0.0, T1=1.0)                                                                # neither form
    bad_cat = [dict(position_m=np.ones((4, 2))), dict(velocity_m_s=np.ones((3, 3))), dict(T1=0.0), dict(n=1), dict(n=2.5),
               dict(position_m=np.zeros((4, 3))), dict(velocity_m_s=np.full((4, 3), np.nan))]
    for kw in bad_cat:
        args = dict(position_m=np.full((4, 3), 7e6), velocity_m_s=np.ones((4, 3)), T0=0.0, T1=100.0, n=10); args.update(kw)
        with pytest.raises(ValueError):
            cj.catalogue_trajectories(**args)


def test_constellation_hands_the_catalogue_through_with_its_own_windows(monkeypatch):
    mpc, _ = hand_made_mpc()
    cat = (np.zeros((4, 7, 9)), np.ones((4, 2)), np.array([[0.0, 1.0]] * 4))
    seen = []

    def fake(**kw):
        seen.append(kw)
        k = len(seen)
        return cj.ConjunctionResult(np.full(3, 10.0 * k), np.full(3, k, dtype=np.int32), np.full(3, float(k)), cj.sort_pairs([[2, k - 1, 10.0 * k, float(k)]]), 1)
    monkeypatch.setattr(cj, "screen_against", fake)
    r = mpc.screen_against(cat, 1000.0, samples_per_node=3)
    win = mpc._screen_windows("flown", samples_per_node=3)
    assert len(seen) == len(win) == 2
    for kw, w in zip(seen, win):
        assert kw["cat_Y"] is cat[0] and kw["cat_units"] is cat[1] and kw["cat_span"] is cat[2] and "cat_ns" not in kw
        assert kw["Y"] is w["Y"] and kw["ns"] is None and np.array_equal(kw["units"], w["units"]) and np.array_equal(kw["span"], w["span"])
        assert (kw["M"], kw["T0"], kw["T1"]) == (w["M"], w["T0"], w["T1"]) and kw["threshold"] == 1000.0 and "max_pairs" not in kw
        assert kw["device"] == mpc.device and kw["devices"] == mpc.devices
    # the two windows joined with combine: the first window's smaller distance, both windows' pairs
    assert r.dmin.tolist() == [10.0] * 3 and r.partner.tolist() == [1] * 3 and r.pairs[:, :2].tolist() == [[2, 0], [2, 1]]
    seen.clear()
    ns = np.full(4, 9, dtype=np.int32)
    mpc.screen_against(cat + (ns,), 5.0, samples_per_node=1, T0=10.0, T1=20.0, max_pairs=7)
    assert all(kw["cat_ns"] is ns and kw["max_pairs"] == 7 and (kw["T0"], kw["T1"]) == (10.0, 20.0) for kw in seen) and len(seen) == 2
    with pytest.raises(ValueError, match="catalogue"):
        mpc.screen_against(cat[:2], 5.0)
    with pytest.raises(ValueError, match="flown.*plan"):
        mpc.screen_against(cat, 5.0, what="planned")


def test_combine_and_sort_keep_pairs_with_j_below_i():
    p = np.array([[3, 1, 10.0, 1.0], [0, 9, 20.0, 2.0], [3, 0, 30.0, 3.0], [5, 2, 40.0, 4.0]])
    assert cj.sort_pairs(p)[:, :2].tolist() == [[0, 9], [3, 0], [3, 1], [5, 2]]
    inf, nan = np.inf, np.nan
    a = cj.ConjunctionResult(np.array([inf, 5.0, 7.0]), np.array([-1, 0, 4], dtype=np.int32), np.array([nan, 1.0, 2.0]),
                             cj.sort_pairs([[1, 0, 5.0, 1.0], [2, 4, 7.0, 2.0]]), 2)
    b = cj.ConjunctionResult(np.array([9.0, 6.0, 7.0]), np.array([2, 0, 1], dtype=np.int32), np.array([11.0, 12.0, 13.0]),
                             cj.sort_pairs([[2, 1, 7.0, 13.0], [1, 0, 6.0, 12.0], [0, 2, 9.0, 11.0]]), 3)
    c = cj.combine([a, b])
    # row 0: only the second window; row 1: the first window is closer; row 2: equal distance, the smaller catalogue index wins
    assert c.dmin.tolist() == [9.0, 5.0, 7.0] and c.partner.tolist() == [2, 0, 1] and c.tca.tolist() == [11.0, 1.0, 13.0]
    assert c.pairs.tolist() == [[0, 2, 9.0, 11.0], [1, 0, 5.0, 1.0], [2, 1, 7.0, 13.0], [2, 4, 7.0, 2.0]] and c.n_pairs_total == 4
    assert c.cat_status is None and a.cat_status is None
    assert cj.ConjunctionResult(a.dmin, a.partner, a.tca, a.pairs, 2, cat_status=np.zeros(5, dtype=np.int32)).cat_status.shape == (5,)
