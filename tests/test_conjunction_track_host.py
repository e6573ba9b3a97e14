"""Following each listed encounter through the re-screens, without a GPU: the restatements (conjunction_track_reference.py) on the
smallest scene that needs it -- a coasting arc and one object whose orbits cross twice inside the span, so that pair (0, 0) has two
events -- where the untracked loop (avoidance_refine_reference.refine, re-screen = the pair's global minimum) gives both rows the
same encounter and fails, and the tracked one brings both to the target; the two loops on the existing one-event scenes, where they
must agree; and screen_track / avoidance_refine(track=...) in front of the library: argument checks and the empty list."""
import numpy as np
import pytest

import avoidance_joint_reference as J
import conjunction_events_reference as E
import conjunction_reference as CJ
import conjunction_track_reference as T
from test_avoidance_joint_host import three_encounters, TARGET
from test_avoidance_refine_host import arc_loop, arc_grid, coupled_scene, coupled_loop, LOOP_BOUND, ROUNDS

assert T.TARGET == TARGET and T.ROUNDS == ROUNDS


def near(got, want, digits):
    """`got` is `want` to the digits `want` is printed with (half a unit of the last one, and the rounding of the print)"""
    return np.all(np.abs(np.asarray(got) - np.asarray(want)) <= 0.5000001 * 10.0 ** -digits)


# ---------------------------------------------------------------- the two-event scene
def test_the_scene_has_two_events_in_two_chunks():
    s = T.two_event_scene()
    p = s["ref"]
    print(f"events of pair (0, 0): intervals {p.interval}, d {p.d}, t {p.t}, edge {p.edge}")
    assert s["grid"][0] == 117 and p.count == 2 and p.interval.tolist() == [17, 89] and not p.edge.any()
    assert p.interval[0] // 64 != p.interval[1] // 64                # two different 64-interval chunks
    assert near(p.d, [184.76, 771.95], 2) and near(p.t, [699.42, 3613.74], 2)
    assert s["pairs"].shape == (2, 4) and not s["U"].any()


def test_untracked_rows_of_one_pair_collapse_onto_its_global_minimum():
    """re-screen = pair_minima: from pass 1 on both rows read the pair's global minimum; with the hold the two identical rows make
    the third solve singular, without it the second encounter is never looked at again"""
    r = T.two_event_loop(False, True)
    print(f"hold: status {r['sat_status']}, rounds_done {r['rounds_done']}\nd0\n{r['d0_history']}\ntca\n{r['tca_history']}")
    assert r["sat_status"].tolist() == [J.ST_SINGULAR] and J.ST_SINGULAR == 4 and r["rounds_done"].tolist() == [2]
    assert np.array_equal(r["d0_history"][1:, 0], r["d0_history"][1:, 1]) and np.array_equal(r["tca_history"][1:, 0], r["tca_history"][1:, 1])
    assert near(r["d0_history"][1:4, 0], [1055.95, 1016.48, 1002.88], 2) and near(r["tca_history"][1:4, 0], [699.395, 699.402, 699.405], 3)
    r = T.two_event_loop(False, False)
    print(f"no hold: status {r['sat_status']}, rounds_done {r['rounds_done']}, flown {r['pairs_flown'].tolist()}")
    assert r["sat_status"].tolist() == [0] and r["rounds_done"].tolist() == [ROUNDS]
    assert np.array_equal(r["pairs_flown"][0], r["pairs_flown"][1])
    assert near(r["pairs_flown"][:, 2], [1000.08, 1000.08], 2) and near(r["pairs_flown"][:, 3], [699.417, 699.417], 3)


def test_tracked_rows_follow_their_own_encounters():
    s = T.two_event_scene()
    r = T.two_event_loop(True, True)
    print(f"hold: status {r['sat_status']}, rounds_done {r['rounds_done']}\nd0\n{r['d0_history']}\ntca\n{r['tca_history']}\n"
          f"terminal {r['terminal_history'][:, 0]}\neffort {r['cost_history'][:, 0]}")
    assert r["sat_status"].tolist() == [0] and r["rounds_done"].tolist() == [ROUNDS]
    assert near(r["d0_history"][:4], [[184.76, 771.95], [1055.95, 1227.05], [1016.48, 1111.24], [1002.88, 1055.12]], 2)
    assert near(r["d0_history"][4], [1000.449, 1034.207], 3)
    assert near(r["tca_history"][-1], [699.406, 3613.717], 3)
    assert abs(r["terminal_history"][-1, 0] - 1.2e-7) <= 0.05e-7
    assert near(1e3 * r["cost_history"][:, 0], [4.90, 3.96, 3.74, 3.71], 2)
    # the end state: both rows at or beyond the target within the refined loop's bound, at their own times
    assert (r["d0_history"][-1] >= TARGET * (1.0 - LOOP_BOUND[(True, True)]["shortfall"])).all() and LOOP_BOUND[(True, True)]["shortfall"] == 3.0 * 6.665e-6
    assert (np.abs(r["tca_history"] - s["pairs"][:, 3]) <= 1.0).all()
    assert r["terminal_history"][-1, 0] <= 3.0 * 1.18e-7
    r = T.two_event_loop(True, False)
    print(f"no hold: flown {r['pairs_flown'].tolist()}")
    assert r["sat_status"].tolist() == [0] and r["rounds_done"].tolist() == [ROUNDS]
    assert near(r["pairs_flown"][:, 2], [1000.08, 11248.3], 1) and near(r["pairs_flown"][0, 2], 1000.08, 2) and near(r["pairs_flown"][1, 3], 3612.94, 2)


# ---------------------------------------------------------------- the existing scenes: one event per row within reach
def test_tracked_and_untracked_agree_where_every_row_is_its_pairs_only_event():
    """three_encounters() (hold, ball) and coupled_scene(): every row's own encounter is its pair's global minimum in every pass, so
    the two re-screens differ only in where their Newton steps start from -- measured 2.1e-8 m and 3.6e-12 s"""
    sc, pairs, rows, stage, cat = three_encounters()
    ref, u_max = arc_loop(True, True)
    got = T.refine_tracked(pairs, None, rows, sc["U"][None], sc["consts"][None], TARGET, arc_grid(), ROUNDS, cat=cat, u_max=u_max, hold_terminal=True)
    cp, cm, crows, cU, cconsts, cgrid = coupled_scene()
    cref = coupled_loop(ROUNDS)
    cgot = T.refine_tracked(cp, cm, crows, cU, cconsts, TARGET, cgrid, ROUNDS, hold_terminal=True)
    for name, a, b in (("arc", got, ref), ("coupled", cgot, cref)):
        dd, dt = np.abs(a["d0_history"] - b["d0_history"]).max(), np.abs(a["tca_history"] - b["tca_history"]).max()
        print(f"{name}: |tracked - untracked| d0 {dd:.3e} m, tca {dt:.3e} s, pairs_flown {np.abs(a['pairs_flown'] - b['pairs_flown']).max():.3e}")
        assert a["sat_status"].tolist() == b["sat_status"].tolist() and a["rounds_done"].tolist() == b["rounds_done"].tolist()
        assert dd <= 1e-6 and dt <= 1e-9 and np.abs(a["pairs_flown"][:, 2] - b["pairs_flown"][:, 2]).max() <= 1e-6
    # why: on the given trajectories every row's nearest event is close to its time and the next one far away
    M, T0, T1 = arc_grid()
    eph, _ = CJ.ephemeris(*rows[:3], M, T0, T1)
    ceph, _ = CJ.ephemeris(cat[0], cat[1], cat[2], M, T0, T1)
    tr = T.track(pairs, eph, T0, T1, ceph)
    ceph2, _ = CJ.ephemeris(*crows[:3], *cgrid)
    tr2 = T.track(cp, ceph2, cgrid[1], cgrid[2])
    for t, given in ((tr, pairs), (tr2, cp)):
        print(f"    nearest event {np.abs(t['out'][:, 3] - given[:, 3])} s from the row's time, the next {t['margin']} s further")
        assert (np.abs(t["out"][:, 3] - given[:, 3]) <= 0.2).all() and (t["margin"] >= 2000.0).all()


# ---------------------------------------------------------------- the restatement of the tracking itself
def test_track_restatement_rules():
    """ties go to the earlier interval, max_shift cuts, a time outside the grid picks the first or last event, bad rows"""
    tg = np.linspace(0.0, 10.0, 11)
    q = np.array([9.0, 4.0, 9.0, 9.0, 4.0, 9.0, 16.0, 1.0, np.inf, np.inf])
    t = tg[:-1] + 0.5
    ref = {(0, 1): E.PairEvents(q, t, tg)}
    assert ref[(0, 1)].interval.tolist() == [1, 4, 7]
    rows = np.array([[0, 1, 0, 3.0], [1, 0, 0, 3.0], [0, 1, 0, -50.0], [0, 1, 0, 99.0], [0, 1, 0, 2.9], [0, 2, 0, 1.0],
                     [0, 1, 0, np.nan], [0, 0, 0, 1.0], [0.5, 1, 0, 1.0], [0, 1, 0, np.inf], [3, 1, 0, 1.0]])
    r = T.track_rows(rows, ref, 3)
    assert r["info"][:, 0].tolist() == [1, 1, 1, 7, 1, -1, -1, -1, -1, -1, -1] and r["status"].tolist() == [0, 0, 0, 0, 0, 0, 9, 9, 9, 9, 9]
    assert r["out"][0, 2:].tolist() == [2.0, 1.5] and r["margin"][0] == 0.0 and np.isposinf(r["out"][5, 2]) and np.isnan(r["out"][5, 3])
    assert np.isnan(r["out"][6:, 2:]).all() and np.array_equal(r["out"][:, :2], rows[:, :2])
    cut = T.track_rows(rows[:5], ref, 3, max_shift=1.45)
    assert cut["info"][:, 0].tolist() == [-1, -1, -1, -1, 1] and np.isposinf(cut["out"][:4, 2]).all() and cut["status"].tolist() == [0] * 5
    assert abs(cut["boundary"][0] - 0.05) <= 1e-12 and abs(cut["boundary"][4] - 0.05) <= 1e-12
    for free in (None, 0.0, -1.0):
        assert T.track_rows(rows, ref, 3, max_shift=free)["out"].tobytes() == r["out"].tobytes()
    # against a catalogue i == j is a pair like any other and (i, j) is not (j, i)
    rc = T.track_rows(np.array([[1, 1, 0, 3.0], [1, 0, 0, 3.0]]), {(1, 1): ref[(0, 1)]}, 3, D=2)
    assert rc["info"][:, 0].tolist() == [1, -1] and rc["status"].tolist() == [0, 0]


# ---------------------------------------------------------------- the wrappers in front of the library
def sides():
    eph, cat = np.zeros((3, 6, 5)), np.zeros((4, 6, 5))
    traj = dict(Y=np.zeros((3, 7, 8)), units=np.ones((3, 2)), span=np.tile([0.0, 1.0], (3, 1)))
    return eph, cat, traj


def test_screen_track_checks_its_arguments_and_answers_an_empty_list_itself():
    from mpconstellation_amd import screen_track, ConjunctionResult, EncounterEvents
    eph, cat, traj = sides()
    one = np.zeros((1, 4))
    for bad, kw in ((np.zeros((2, 3)), dict(eph=eph)), (one, dict()), (one, dict(eph=eph, M=5, **traj)), (one, dict(cat_eph=cat)),
                    (one, dict(eph=eph, cat_eph=np.zeros((4, 6, 6)))), (one, dict(eph=eph, M=4)), (one, dict(**traj)), (one, dict(M=1, **traj)),
                    (one, dict(eph=eph, max_shift=np.nan)), (one, dict(eph=eph, max_shift=[1.0, 2.0])),
                    (np.zeros((0, 4)), dict(eph=eph, max_shift=np.nan))):    # (an empty list is checked like any other)
        with pytest.raises(ValueError):
            screen_track(bad, 0.0, 1.0, **kw)
    with pytest.raises(ValueError, match="screen_track"):
        screen_track(one, 0.0, 1.0)
    with pytest.raises(ValueError, match="max_shift"):
        screen_track(one, 0.0, 1.0, eph=eph, max_shift=np.nan)
    with pytest.raises(ValueError):
        screen_track(one, 1.0, 1.0, eph=eph)
    out, info, status = screen_track(np.zeros((0, 4)), 0.0, 1.0, max_shift=5.0, eph=eph, cat_eph=cat)
    assert out.shape == (0, 4) and out.dtype == np.float64 and info.shape == (0, 2) and info.dtype == np.int32
    assert status.shape == (0,) and status.dtype == np.int32
    empty = ConjunctionResult(np.zeros(3), np.zeros(3, dtype=np.int32), np.zeros(3), np.zeros((0, 4)), 0)
    got = screen_track(empty, 0.0, 1.0, M=5, **traj)
    assert len(got) == 5 and got[0].shape == (0, 4) and got[3] is None and got[4] is None
    ev = EncounterEvents(np.zeros((0, 3, 4)), np.zeros((0, 3, 2), dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32))
    assert screen_track(ev, 0.0, 1.0, eph=eph)[0].shape == (0, 4)


def test_avoidance_refine_checks_track_and_max_shift():
    from mpconstellation_amd import avoidance_refine, AvoidanceRefineResult
    S, K = 3, 5
    plan = dict(Y=np.ones((S, 7, K)), U=np.zeros((S, 3, K)), units=np.ones((S, 2)), span=np.array([[0.0, 1.0]] * S), consts=np.ones((S, 8)))
    grid = dict(M=9, T0=0.0, T1=1.0)
    pairs = np.array([[0.0, 1.0, 10.0, 0.5], [0.0, 1.0, 10.0, 0.7]])
    for bad in (np.nan, [1.0, 2.0]):
        with pytest.raises(ValueError, match="max_shift"):
            avoidance_refine(pairs, 100.0, **plan, **grid, track=True, max_shift=bad)
        with pytest.raises(ValueError, match="max_shift"):          # (an empty list is checked like any other)
            avoidance_refine(np.zeros((0, 4)), 100.0, **plan, **grid, track=True, max_shift=bad)
    with pytest.raises(ValueError, match="one device"):
        avoidance_refine(pairs, 100.0, **plan, **grid, track=True, devices=[0, 1])
    res = avoidance_refine(np.zeros((0, 4)), 100.0, **plan, **grid, rounds=2, track=True, max_shift=30.0)
    assert isinstance(res, AvoidanceRefineResult) and res.pairs_flown.shape == (0, 4) and res.d0_history.shape == (4, 0)
    assert res.rounds_done.tolist() == [-1] * S and not res.du.any()
    assert avoidance_refine(np.zeros((0, 4)), 100.0, **plan, **grid, track=False, max_shift=np.nan).du.shape == (S, 3, K)   # read only with track


def test_the_binding_and_the_exports_name_the_new_entry_points():
    import mpconstellation_amd as pkg
    from mpconstellation_amd import _ffi, ConstellationMPC
    names = {"mpcx_conjunction_track" + tail for tail in ("", "_dev", "_traj", "_traj_dev", "_workspace_bytes")}
    names |= {"mpcx_avoidance_refine_tracked", "mpcx_avoidance_refine_tracked_dev"}
    assert names <= set(_ffi.exported_symbols())
    assert "screen_track" in pkg.__all__ and callable(pkg.screen_track)
    args = ConstellationMPC.avoidance_refine.__code__.co_varnames
    assert "events" in args and "max_events" in args
