"""The iterated avoidance that follows its rows (mpcx_avoidance_refine_tracked in csrc/avoidance_joint.hip: the loop of
mpcx_avoidance_refine with mpcx_conjunction_track_traj_dev of the GIVEN list as its re-screen) on the device: with rounds = 0 the
chain of public calls it is made of, bit for bit; the two-event scene of test_conjunction_track_host.py -- one pair listed twice,
once per encounter -- against the restatement (conjunction_track_reference.refine_tracked) and beside the untracked call, whose two
rows collapse onto one encounter; the existing one-event scenes, where tracking must not change a bit; ConstellationMPC."""
import functools

import numpy as np
import pytest

import avoidance_reference as AR
import conjunction_track_reference as T
from dev_solve import same_bits
from test_avoidance_gpu import arc_on_device
from test_avoidance_joint_host import three_encounters, TARGET
from test_avoidance_refine_host import arc_loop, arc_grid, coupled_scene, LOOP_BOUND, ROUNDS
from test_avoidance_refine_gpu import bits

pytestmark = pytest.mark.gpu

ALL_OUTPUTS = ("du", "sat_out", "row_out", "rows", "tsens", "status", "row_status", "Y_flown", "pairs_flown", "d0_history", "tca_history",
               "terminal_history", "rounds_done", "rhs_rows", "rhs_term")


@functools.lru_cache(maxsize=None)
def scene_on_device():
    """the two-event scene with the coasting arc as the device flies it, and its two restated events as the list"""
    s = T.two_events(T.coasting_arc(fly=arc_on_device))
    assert s["ref"].count == 2 and s["ref"].interval.tolist() == [17, 89]
    return s


def refine(s, rounds, track, hold=True, **kw):
    from mpconstellation_amd import avoidance_refine
    Y, units, span, _ = s["rows"]
    M, T0, T1 = s["grid"]
    return avoidance_refine(s["pairs"], TARGET, Y, s["U"], units, span, s["consts"], M, T0, T1, rounds=rounds, cat=s["cat"][:3], hold_terminal=hold,
                            prop_max_step=AR.SCENE["prop_max_step"], track=track, return_rows=True, return_terminal=True, return_rhs=True, **kw)


@functools.lru_cache(maxsize=None)
def two_events_refined(track):
    return refine(scene_on_device(), ROUNDS, track)


# ---------------------------------------------------------------- rounds = 0: the chain through public calls
def test_rounds_zero_is_the_chain_of_public_calls():
    """rounds = 0 with track=True: avoidance_joint's bits, then Y_flown = propagate_batch under U + du, pairs_flown = screen_track of
    the GIVEN list on it (two rows of one pair, two different encounters -- screen_pairs gives both the same one), d0_history[1] =
    avoidance_joint(pairs_flown, Y_flown, U + du).d0"""
    from mpconstellation_amd import avoidance_joint, propagate_batch, screen_pairs, screen_track, _ffi
    s = scene_on_device()
    Y, units, span, _ = s["rows"]
    M, T0, T1 = s["grid"]
    K = Y.shape[2]
    cY, cunits, cspan = s["cat"][:3]
    res = refine(s, 0, True)
    ref = avoidance_joint(s["pairs"], TARGET, Y, s["U"], units, span, s["consts"], cat=s["cat"][:3], hold_terminal=True, return_rows=True,
                          return_terminal=True)
    print(f"status {ref.status.tolist()}, rows {ref.n_rows.tolist()}, d0 {res.d0_history.tolist()}, tca {res.tca_history.tolist()}, terminal {res.terminal_history.tolist()}")
    for name in ("du", "sat_out", "row_out", "rows", "tsens", "row_status", "status"):
        assert same_bits(getattr(res, name), getattr(ref, name)), name
    assert ref.status.tolist() == [0] and ref.n_rows.tolist() == [2] and res.rounds_done.tolist() == [0]
    assert same_bits(res.rhs_rows, TARGET - ref.d0) and not res.rhs_term.any()
    # the flight
    Ut = s["U"] + ref.du
    tf = (span[:, 1] - span[:, 0]) / units[:, 1]
    y, st, _ = propagate_batch(np.ascontiguousarray(Y[:, :, 0]), tf, s["consts"], (_ffi.CTRL_SEQUENCE, Ut, K, 1.0), K, max_step=AR.SCENE["prop_max_step"])
    assert st.tolist() == [0] and same_bits(res.Y_flown, y)
    term = np.abs(y[0, :6, K - 1] - Y[0, :6, K - 1]).max()
    assert same_bits(res.terminal_history, np.array([[0.0], [term]])) and term > 0.0
    # the re-screen: every row its own encounter
    side = dict(Y=y, units=units, span=span, M=M, cat_Y=cY, cat_units=cunits, cat_span=cspan)
    again = screen_track(s["pairs"], T0, T1, **side)[0]
    assert same_bits(res.pairs_flown, again) and same_bits(res.tca_history, np.stack([s["pairs"][:, 3], again[:, 3]]))
    assert (np.abs(again[:, 3] - s["pairs"][:, 3]) <= 1.0).all() and again[1, 3] - again[0, 3] > 2000.0
    closest = screen_pairs(s["pairs"], T0, T1, **side)[0]
    assert closest[0].tobytes() == closest[1].tobytes() and min(again[:, 2]) == closest[0, 2]      # (what the untracked loop would read)
    # the rows of the flown state
    flown = avoidance_joint(again, TARGET, y, Ut, units, span, s["consts"], cat=s["cat"][:3], hold_terminal=True)
    assert same_bits(res.d0_history, np.stack([ref.d0, flown.d0]))


# ---------------------------------------------------------------- the two-event scene, refined
# |device - restatement| measured on the first run on an MI355X (the test prints them), asserted at 3 x.  As in
# test_avoidance_refine_gpu.py the two differ in their integrators (the device's discretiser and flight against the CPU oracle's) and
# in the arc itself, which the device flies here and the oracle there -- and with it in the planted object and the list.
# (profiles/avoidance_refine_tracked.txt)
#   d0 history 1.47e-8 m, tca history 1.82e-12 s, terminal history 4.85e-14, final du / max |du| 1.05e-12
DEVICE_MEASURED = dict(d0=1.47e-8, tca=1.82e-12, term=4.85e-14, du=1.05e-12)


def allowed(key):
    m = DEVICE_MEASURED[key]
    assert m is not None, f"{key}: no measured figure recorded yet (see the printed differences)"
    return 3.0 * m


def test_two_events_tracked_against_the_restatement():
    """track=True, rounds = 3, the hold: both rows at or beyond the target within the refined loop's bound, each at its own time;
    histories and du against the restatement within 3 x the measured differences"""
    s = scene_on_device()
    res = two_events_refined(True)
    ref = T.two_event_loop(True, True)
    diff = dict(d0=np.abs(res.d0_history - ref["d0_history"]).max(), tca=np.abs(res.tca_history - ref["tca_history"]).max(),
                term=np.abs(res.terminal_history - ref["terminal_history"]).max(), du=np.abs(res.du - ref["du"]).max() / np.abs(ref["du"]).max())
    print(f"status {res.status.tolist()}, rounds_done {res.rounds_done.tolist()}, iterations of the last solve {res.iters.tolist()}\nd0 by pass\n{res.d0_history}\n"
          f"tca by pass\n{res.tca_history}\nterminal deviation by pass {res.terminal_history[:, 0]}\npairs_flown\n{res.pairs_flown}\n|device - restatement|: {diff}")
    assert res.status.tolist() == [0] and res.rounds_done.tolist() == [ROUNDS] and (res.row_status == 0).all()
    assert res.pairs_flown[0, 3] != res.pairs_flown[1, 3] and (np.abs(res.pairs_flown[:, 3] - s["pairs"][:, 3]) <= 1.0).all()
    assert (np.abs(res.tca_history - s["pairs"][:, 3]) <= 1.0).all()
    assert LOOP_BOUND[(True, True)]["shortfall"] == 3.0 * 6.665e-6 and (res.d0_history[-1] >= TARGET * (1.0 - LOOP_BOUND[(True, True)]["shortfall"])).all()
    for k, d in diff.items():
        assert d <= allowed(k), (k, d)


def test_two_events_untracked_rows_collapse():
    """track=False on the same list: from pass 1 on both rows of one pair carry the pair's global minimum, byte for byte -- what
    tracking changes.  (Under the hold the two identical rows make a later solve singular; the status is printed, not asserted:
    which solve fails depends on a pivot at rounding level.)"""
    res, tracked = two_events_refined(False), two_events_refined(True)
    print(f"status {res.status.tolist()}, rounds_done {res.rounds_done.tolist()}\nd0 by pass\n{res.d0_history}\ntca by pass\n{res.tca_history}")
    assert res.pairs_flown[0].tobytes() == res.pairs_flown[1].tobytes()
    assert res.d0_history[1:, 0].tobytes() == res.d0_history[1:, 1].tobytes() and res.tca_history[1:, 0].tobytes() == res.tca_history[1:, 1].tobytes()
    assert abs(res.pairs_flown[0, 3] - scene_on_device()["pairs"][0, 3]) <= 1.0          # both read the first encounter
    # pass 0 and the first flight are the same call; the first re-screen's row 0 is the same event
    assert same_bits(res.d0_history[0], tracked.d0_history[0]) and res.d0_history[1, 0] == tracked.d0_history[1, 0]
    assert tracked.d0_history[1, 1] != res.d0_history[1, 1]


# ---------------------------------------------------------------- the existing scenes: tracking changes no bit
def same_outputs(a, b):
    for name in ALL_OUTPUTS:
        assert same_bits(getattr(a, name), getattr(b, name)), name


def test_three_encounters_same_bytes():
    """three_encounters() on the arc as the device flies it, the hold and the ball of the host loop: every row's own encounter is its
    pair's smallest event, and both re-screens take (q, t) of an interval from cj_interval on that interval alone"""
    from mpconstellation_amd import avoidance_refine
    sc, pairs, rows, stage, cat = three_encounters()
    _, u_max = arc_loop(True, True, ROUNDS)
    x = arc_on_device(sc["U"])
    M, T0, T1 = arc_grid()
    run = lambda **kw: avoidance_refine(pairs, TARGET, x[None], sc["U"][None], sc["units"][None], sc["span"][None], sc["consts"][None], M, T0, T1,
                                        rounds=ROUNDS, cat=cat[:3], u_max=u_max, hold_terminal=True, prop_max_step=AR.SCENE["prop_max_step"],
                                        return_rows=True, return_terminal=True, return_rhs=True, **kw)
    a, b = run(track=False), run(track=True)
    assert a.status.tolist() == [0] and a.rounds_done.tolist() == [ROUNDS]
    same_outputs(a, b)
    same_outputs(a, run(track=True, max_shift=60.0))
    assert bits(a) == bits(run())                                    # (the default is the untracked call)


def test_coupled_scene_same_bytes():
    from mpconstellation_amd import avoidance_refine
    pairs, mover, (Y, units, span, _), U, consts, (M, T0, T1) = coupled_scene()
    run = lambda **kw: avoidance_refine(pairs, TARGET, Y, U, units, span, consts, M, T0, T1, rounds=ROUNDS, who=mover, hold_terminal=True,
                                        prop_max_step=AR.SCENE["prop_max_step"], return_rows=True, return_terminal=True, return_rhs=True, **kw)
    a, b = run(track=False), run(track=True)
    assert a.status.tolist() == [0, 0, 0] and a.rounds_done.tolist() == [3, 3, -1]
    same_outputs(a, b)


def test_a_row_that_loses_its_event_freezes_its_satellite():
    """max_shift so small that the flown encounters lie outside it: the re-screen's rows are (+inf, NaN), the solve of pass 1 fails
    with MPCX_ST_BADK, the satellite keeps the manoeuvre of pass 0 and goes on flying it -- the path of a row without a valid
    interval in the untracked call (include/mpcx.h)"""
    s = scene_on_device()
    r0 = refine(s, 0, True)
    shifts = np.abs(r0.pairs_flown[:, 3] - s["pairs"][:, 3])
    limit = 0.5 * shifts.min()
    assert limit > 1e-4
    res = refine(s, 2, True, max_shift=limit)
    print(f"shifts after the first flight {shifts} s, max_shift {limit} s: status {res.status.tolist()}, rounds_done {res.rounds_done.tolist()}, pairs_flown {res.pairs_flown.tolist()}")
    assert res.status.tolist() == [9] and res.rounds_done.tolist() == [0]
    assert np.isposinf(res.pairs_flown[:, 2]).all() and np.isnan(res.pairs_flown[:, 3]).all() and np.isnan(res.tca_history[1:]).all()
    assert same_bits(res.du, r0.du) and same_bits(res.sat_out, r0.sat_out) and same_bits(res.row_out, r0.row_out) and same_bits(res.Y_flown, r0.Y_flown)
    assert same_bits(res.terminal_history[1:], np.repeat(r0.terminal_history[1:], 3, axis=0))


# ---------------------------------------------------------------- ConstellationMPC
# The plan's events (printed below), in 1e6 m: pair (0, 1) 10.44 at t = 0 (an edge event), 8.20, 8.41, 13.65; pair (0, 2) 11.73 at
# t = 0, 9.94, 10.00; pair (1, 2) 11.19 at t = 0, 11.39, 11.98.  At 10.2e6 m the list is two pairs with two events each, none of
# them an edge event, four rows of satellite 0; the target lies above the two events of pair (0, 1) and below those of (0, 2).
MPC_THRESHOLD = 1.02e7
MPC_TARGET = 8.5e6


def test_constellation_mpc_refines_every_event():
    """Three satellites, one update over a horizon of two time units (test_conjunction_events_gpu.py's instance):
    ConstellationMPC.avoidance_refine(events=True) returns, bit for bit, what the module-level chain returns -- encounters' list, then
    conjunction.avoidance_refine(events.events, track=True) with the instance's thrust limit -- and install=True puts the refined
    plan where fly_plan takes it from"""
    from mpconstellation_amd import Satellite, ConstellationMPC, conjunction as cj, _ffi
    from mpconstellation_amd.constellation import constellation_states
    from mpconstellation_amd.optimizer import DEFAULT_OPTIONS
    from test_conjunction_events_gpu import bits as event_bits
    st = constellation_states(3)
    mpc = ConstellationMPC([Satellite(s[:3].copy(), s[3:6].copy(), float(s[6])) for s in st], base_res=30, tf_horizon=2, tf_interval=1, r_des=1.5)
    mpc.update()
    (w,) = mpc._screen_windows("plan", samples_per_node=4)
    everything = mpc.encounters(1e12, max_events=16)[1]
    print(f"every event of the plan: per pair {everything.count.tolist()}\n{everything.events}")
    U0 = mpc._plan[1].copy()
    scr, ev, res = mpc.avoidance_refine(MPC_THRESHOLD, MPC_TARGET, rounds=2, events=True, max_events=8)
    scr2, ev2 = mpc.encounters(MPC_THRESHOLD, max_events=8)
    rows_per_mover = np.bincount(ev.events[:, 0].astype(int), minlength=3)
    print(f"threshold {MPC_THRESHOLD}: pairs {scr.pairs[:, :2].tolist()}, events per pair {ev.count.tolist()}, rows per mover {rows_per_mover.tolist()}, "
          f"status {res.status.tolist()}, rounds_done {res.rounds_done.tolist()}\nd0 by pass\n{res.d0_history}")
    assert ev.count.max() >= 2 and rows_per_mover.max() <= _ffi.AJ_MAX_ROWS and not ev.truncated.any()
    assert ev.count.tolist() == [2, 2] and not ev.edge.any() and res.status.tolist() == [0, 0, 0] and res.rounds_done.tolist() == [2, -1, -1]
    assert (res.d0_history[0, :2] < MPC_TARGET).all() and (res.d0_history[-1] >= MPC_TARGET * (1.0 - LOOP_BOUND[(True, True)]["shortfall"])).all()
    # every row near the time it was listed at, and the two rows of a pair as far apart as its two encounters are
    assert (np.abs(res.tca_history[-1] - ev.events[:, 3]) <= 100.0).all() and (ev.events[[1, 3], 3] - ev.events[[0, 2], 3] > 2000.0).all()
    assert (res.pairs_flown[[1, 3], 3] - res.pairs_flown[[0, 2], 3] > 2000.0).all()
    assert scr.pairs.tobytes() == scr2.pairs.tobytes() and event_bits(ev) == event_bits(ev2)
    u_lim = np.asarray({**DEFAULT_OPTIONS, **mpc.OPTIONS(mpc.horizon), **mpc.options}["u_lim"], dtype=np.float64)
    u_max = np.ascontiguousarray(np.broadcast_to(u_lim[..., 1], (3,)))
    hand = cj.avoidance_refine(ev2.events, MPC_TARGET, w["Y"], U0, w["units"], w["span"], mpc.consts, w["M"], w["T0"], w["T1"], rounds=2, ns=w["ns"],
                               u_max=u_max, track=True)
    assert bits(res) == bits(hand) and len(res.pairs) == len(ev.events)
    # installed, and flown
    scr3, ev3, res3 = mpc.avoidance_refine(MPC_THRESHOLD, MPC_TARGET, rounds=2, events=True, max_events=8, install=True)
    assert bits(res3) == bits(res)
    ok = (res3.status == 0) & np.isfinite(res3.du).all(axis=(1, 2))
    assert np.array_equal(mpc._plan[1][ok], U0[ok] + res3.du[ok]) and np.array_equal(mpc._plan[1][~ok], U0[~ok]) and same_bits(mpc._plan[0][ok], res3.Y_flown[ok])
    mpc.fly_plan(tf=1)
    assert np.isfinite(mpc._seg_y[-1]).all()
