"""The close approach nearest each listed row's own time on the device (csrc/conjunction.hip: track_kernel, one wave per row,
events_kernel's walk over chunks of 64 consecutive intervals, the minimum under (|t - t_row|, interval) by an xor butterfly) against
  screen_events, byte for byte: every row of its output, given back on the same inputs, returns its own distance, time, interval
    and edge flag -- in every form (ephemerides and trajectories, the list permuted, (j, i), a catalogue, two contexts);
  screen_pairs, byte for byte: a row of its output returns its distance and time;
  the numpy restatement (conjunction_track_reference.py) for times moved towards the neighbouring events, before T0 and after T1,
    with and without max_shift: the same interval and edge, distance within 1e-6 m + 1e-12 d and time within 1e-6 s, the tolerances
    test_conjunction_events_gpu.py holds the events to.  Comparing CHOICES is sound because every event's q is at least 1e-9
    relative from its neighbours' (asserted there and here) and every row's two nearest events differ by at least 1e-3 s in |dt|,
    and its events are at least 1e-3 s from the max_shift boundary (asserted).
The shapes are the events tests' own: events in intervals 63, 64 and 128, the last and the first lane of a chunk."""
import functools

import numpy as np
import pytest

import conjunction_reference as R
import conjunction_events_reference as E
import conjunction_track_reference as T
from test_conjunction_events_gpu import SCENES, S6, S6X9, ALL, full, rows, ragged, of_row

pytestmark = pytest.mark.gpu

MARGIN = 1e-3                                                        # seconds


def assert_fixed_point(got, events, interval, edge):
    out, info, status = got[:3]
    assert out.tobytes() == events.tobytes()
    assert info.dtype == np.int32 and info[:, 0].tobytes() == np.asarray(interval, dtype=np.int32).tobytes()
    assert info[:, 1].tolist() == np.asarray(edge, dtype=int).tolist() and (status == 0).all() and len(out) > 0


# ---------------------------------------------------------------- the fixed point
@pytest.mark.parametrize("M,orbits", SCENES)
def test_an_event_given_back_returns_itself_in_every_form(M, orbits):
    from mpconstellation_amd import common_clock, screen, screen_events, screen_track
    c, ref, listed, ev = full(M, orbits)
    grid = (c["T0"], c["T1"])
    assert not ev.truncated.any() and len(ev.events) == sum(p.count for p in ref.values())
    assert_fixed_point(screen_track(ev.events, *grid, eph=c["eph"]), ev.events, ev.interval, ev.edge)
    assert_fixed_point(screen_track(ev, *grid, eph=c["eph"]), ev.events, ev.interval, ev.edge)          # (the EncounterEvents itself)
    # the list permuted: every row's answer moves with it
    perm = np.random.default_rng(M).permutation(len(ev.events))
    assert_fixed_point(screen_track(ev.events[perm], *grid, eph=c["eph"]), ev.events[perm], ev.interval[perm], ev.edge[perm])
    # (j, i): the same operations on the same operands
    swapped = np.ascontiguousarray(ev.events[:, [1, 0, 2, 3]])
    out, info, status = screen_track(swapped, *grid, eph=c["eph"])
    assert_fixed_point((np.ascontiguousarray(out[:, [1, 0, 2, 3]]), info, status), ev.events, ev.interval, ev.edge)
    # two contexts
    assert_fixed_point(screen_track(ev.events, *grid, eph=c["eph"], devices=[0, 0]), ev.events, ev.interval, ev.edge)
    # from trajectories: the device's own ephemeris; the same bits as common_clock followed by the call
    traj = dict(Y=c["Y"], units=c["units"], span=c["span"], M=M)
    rt = screen(T0=c["T0"], T1=c["T1"], threshold=ALL, **traj)
    evt = screen_events(rt, *grid, max_events=ev.max_events, **traj)
    got = screen_track(evt.events, *grid, **traj)
    assert len(got) == 5 and got[3].tolist() == [0] * 6 and got[4] is None
    assert_fixed_point(got, evt.events, evt.interval, evt.edge)
    assert_fixed_point(screen_track(evt.events, *grid, eph=common_clock(c["Y"], c["units"], c["span"], M, *grid)), evt.events, evt.interval, evt.edge)
    got2 = screen_track(evt.events, *grid, devices=[0, 0], **traj)
    assert_fixed_point(got2, evt.events, evt.interval, evt.edge)
    assert got2[3].tolist() == [0] * 6


@pytest.mark.parametrize("M", [17, 66])
def test_fixed_point_against_a_catalogue(M):
    from mpconstellation_amd import screen_against, screen_events, screen_pairs, screen_track
    c, ref = E.cross_case(6, 9, M)
    grid = (c["T0"], c["T1"])
    most = max(p.count for p in ref.values())
    both = dict(eph=c["eph"], cat_eph=c["cat_eph"])
    r = screen_against(c["eph"], c["cat_eph"], *grid, threshold=ALL)
    ev = screen_events(r, *grid, max_events=most, **both)
    assert len(r.pairs) == 54 and not ev.truncated.any()
    assert_fixed_point(screen_track(ev.events, *grid, **both), ev.events, ev.interval, ev.edge)
    perm = np.random.default_rng(M).permutation(len(ev.events))
    assert_fixed_point(screen_track(ev.events[perm], *grid, devices=[0, 0, 0], **both), ev.events[perm], ev.interval[perm], ev.edge[perm])
    # screen_pairs' rows
    out, _ = screen_pairs(r, *grid, **both)
    got = screen_track(out, *grid, **both)
    assert got[0].tobytes() == out.tobytes() and (got[2] == 0).all() and (got[1][:, 0] >= 0).all()
    # from trajectories
    traj = dict(M=M, **c["sat"], **c["cat"])
    rt = screen_against(T0=c["T0"], T1=c["T1"], threshold=ALL, **traj)
    evt = screen_events(rt, *grid, max_events=most, **traj)
    got = screen_track(evt.events, *grid, **traj)
    assert got[3].tolist() == [0] * 6 and got[4].tolist() == [0] * 9
    assert_fixed_point(got, evt.events, evt.interval, evt.edge)
    assert_fixed_point(screen_track(evt.events, *grid, devices=[0, 0], **traj), evt.events, evt.interval, evt.edge)


@pytest.mark.parametrize("M,orbits", SCENES)
def test_a_row_of_screen_pairs_returns_its_distance_and_time(M, orbits):
    from mpconstellation_amd import screen_pairs, screen_track
    c, ref, listed, ev = full(M, orbits)
    out, _ = screen_pairs(listed, c["T0"], c["T1"], eph=c["eph"])
    got, info, status = screen_track(out, c["T0"], c["T1"], eph=c["eph"])
    assert got.tobytes() == out.tobytes() == listed.tobytes() and (status == 0).all()
    for k in range(len(out)):                                        # (the pair's smallest event, the earliest of equal ones)
        e, m, _ = of_row(ev, k)
        assert info[k, 0] == m[int(np.argmin(e[:, 2]))]


# ---------------------------------------------------------------- moved times against the restatement
def moved_rows(ref, T0, T1, swap_every=3):
    """for every event with a later neighbour at spacing D: a row at t_e + 0.4 D (the event wins), at t_e + 0.6 D (the neighbour
    wins), and at t_l - 0.4 D from the later one towards the earlier (the later wins); per pair one row before T0 and one after T1.
    Every swap_every-th row is given as (j, i) -- all-pairs lists only (swap_every = 0: never)"""
    out = []
    for (i, j), p in sorted(ref.items()):
        ts = [T0 - 777.0, T1 + 777.0] if p.count else []
        for k in range(p.count - 1):
            gap = p.t[k + 1] - p.t[k]
            ts += [p.t[k] + 0.4 * gap, p.t[k] + 0.6 * gap, p.t[k + 1] - 0.4 * gap]
        out += [(i, j, -7.0, t) for t in ts]
    out = np.array(out, dtype=np.float64)
    if swap_every:
        out[::swap_every, :2] = out[::swap_every, 1::-1]
    return out


def assert_matches_restatement(got, want):
    out, info, status = got[:3]
    assert status.tolist() == want["status"].tolist() and info.tolist() == want["info"].tolist()
    assert np.array_equal(out[:, :2], want["out"][:, :2])
    have = info[:, 0] >= 0
    assert np.isposinf(out[~have, 2]).all() and np.isnan(out[~have, 3]).all()
    d, dref = out[have, 2], want["out"][have, 2]
    worst_d = float((np.abs(d - dref) / (1e-6 + 1e-12 * dref)).max()) if have.any() else 0.0
    worst_t = float(np.abs(out[have, 3] - want["out"][have, 3]).max()) if have.any() else 0.0
    print(f"    {len(out)} rows, {int(have.sum())} with an event: worst |d - d_ref| / (1e-6 m + 1e-12 d) {worst_d:.3e}, worst |t - t_ref| {worst_t:.3e} s")
    assert worst_d <= 1.0 and worst_t <= 1e-6


@pytest.mark.parametrize("M,orbits", SCENES)
def test_moved_times_against_the_restatement(M, orbits):
    from mpconstellation_amd import screen_track
    c, ref, listed, ev = full(M, orbits)
    moved = moved_rows(ref, c["T0"], c["T1"])
    want = T.track_rows(moved, ref, 6)
    gap = E.smallest_gap(ref)
    print(f"M {M}: {len(moved)} rows, smallest |dt| margin {want['margin'].min():.3e} s, smallest relative gap of an event's q {gap:.3e}")
    assert gap >= E.GAP and (want["margin"] >= MARGIN).all() and (want["status"] == 0).all()
    if orbits == 3.0:
        assert len(moved) > 15 * 2 + 3 * 15                          # neighbours exist: the three kinds of moved rows are there
        first = np.array([ref[(min(i, j), max(i, j))].interval[0] for i, j in moved[:, :2].astype(int)])
        assert (want["info"][:, 0] != first).any()                   # not always the pair's first event
    assert_matches_restatement(screen_track(moved, c["T0"], c["T1"], eph=c["eph"]), want)
    assert_matches_restatement(screen_track(moved, c["T0"], c["T1"], eph=c["eph"], devices=[0, 0]), want)


@pytest.mark.parametrize("M", [17, 66])
def test_moved_times_against_a_catalogue(M):
    from mpconstellation_amd import screen_track
    c, ref = E.cross_case(6, 9, M)
    moved = moved_rows(ref, c["T0"], c["T1"], swap_every=0)
    want = T.track_rows(moved, ref, 6, 9)
    assert E.smallest_gap(ref) >= E.GAP and (want["margin"] >= MARGIN).all() and len(moved) >= 2 * 54
    assert_matches_restatement(screen_track(moved, c["T0"], c["T1"], eph=c["eph"], cat_eph=c["cat_eph"]), want)


# ---------------------------------------------------------------- max_shift
def a_limit_between(dts):
    """a max_shift in the widest gap between two consecutive distinct |dt| of the list's middle half -> (limit, half the gap)"""
    u = np.unique(dts)
    lo, hi = len(u) // 4, max(3 * len(u) // 4, len(u) // 4 + 2)
    k = lo + int(np.argmax(np.diff(u[lo:hi])))
    return 0.5 * (u[k] + u[k + 1]), 0.5 * (u[k + 1] - u[k])


@pytest.mark.parametrize("M", [65, 66, 130])
def test_max_shift_cuts_the_rows_beyond_it(M):
    from mpconstellation_amd import screen_track
    c, ref, listed, ev = full(M, 3.0)
    grid = (c["T0"], c["T1"])
    moved = moved_rows(ref, *grid)
    free = T.track_rows(moved, ref, 6)
    limit, _ = a_limit_between(np.abs(free["out"][:, 3] - moved[:, 3]))
    want = T.track_rows(moved, ref, 6, max_shift=limit)
    cut = want["info"][:, 0] < 0
    print(f"M {M}: max_shift {limit:.3f} s cuts {int(cut.sum())} of {len(moved)} rows; smallest distance of an event from the boundary {want['boundary'].min():.3e} s")
    assert 0 < cut.sum() < len(cut) and (want["boundary"] >= MARGIN).all() and (want["margin"] >= MARGIN).all()
    got = screen_track(moved, *grid, max_shift=limit, eph=c["eph"])
    assert_matches_restatement(got, want)
    out, info, status = got
    assert np.isposinf(out[cut, 2]).all() and np.isnan(out[cut, 3]).all() and (info[cut] == [-1, 0]).all() and (status == 0).all()
    unlimited = screen_track(moved, *grid, max_shift=1e12, eph=c["eph"])
    assert out[~cut].tobytes() == unlimited[0][~cut].tobytes() and info[~cut].tobytes() == unlimited[1][~cut].tobytes()
    for no_limit in (None, 0.0, -1.0):
        again = screen_track(moved, *grid, max_shift=no_limit, eph=c["eph"])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again, unlimited))
    assert_matches_restatement(unlimited, free)


# ---------------------------------------------------------------- ragged spans
@pytest.mark.parametrize("M", [66, 130])
def test_ragged_spans_and_counts(M):
    from mpconstellation_amd import screen_events, screen_track
    sat, cat, T0, T1 = ragged(M)
    eph, st = R.ephemeris(sat["Y"], sat["units"], sat["span"], M, T0, T1, sat["ns"])
    ceph, cst = R.ephemeris(cat["cat_Y"], cat["cat_units"], cat["cat_span"], M, T0, T1, cat["cat_ns"])
    when = T0 + 0.43 * (T1 - T0)                                     # (not the middle: the spans of the scene are symmetric about it)
    for listed, ref, kw, D in ((rows(S6), E.all_pairs(eph, T0, T1), {}, 0), (rows(S6X9), E.against(eph, ceph, T0, T1), cat, 9)):
        assert E.smallest_gap(ref) >= E.GAP
        most = max(p.count for p in ref.values())
        ev = screen_events(listed, T0, T1, max_events=most, M=M, **sat, **kw)
        # the fixed point, edge events among them
        got = screen_track(ev.events, T0, T1, M=M, **sat, **kw)
        assert_fixed_point(got, ev.events, ev.interval, ev.edge)
        assert ev.edge.any() and got[1][:, 1].sum() == ev.edge.sum()
        assert got[3].tolist() == ev.eph_status.tolist() == st.tolist()
        assert got[4] is None if not kw else got[4].tolist() == ev.cat_status.tolist() == cst.tolist()
        # every listed pair at one time: those never on the grid together and the single-node objects have no event
        asked = listed.copy(); asked[:, 3] = when
        want = T.track_rows(asked, ref, 6, D)
        out, info, status = screen_track(asked, T0, T1, M=M, devices=[0, 0], **sat, **kw)[:3]
        never = np.array([not np.isfinite(ref[(int(i), int(j))].q).any() for i, j in listed[:, :2]])
        assert never.any() and (want["margin"] >= MARGIN).all()
        assert np.isposinf(out[never, 2]).all() and np.isnan(out[never, 3]).all() and (info[never] == [-1, 0]).all() and (status == 0).all()
        assert_matches_restatement((out, info, status), want)
        if not kw:
            at = {(int(i), int(j)): k for k, (i, j) in enumerate(listed[:, :2])}
            assert never[at[(1, 2)]] and all(never[k] for ij, k in at.items() if 3 in ij)      # never together; the single node


# ---------------------------------------------------------------- bad rows and the C ABI
def test_bad_rows_are_reported_and_leave_their_neighbours_alone():
    from mpconstellation_amd import screen_track
    c, ref, listed, ev = full(130, 3.0)
    t = 0.5 * (c["T0"] + c["T1"])
    ij = np.array([(0, 1), (np.nan, 1), (0.5, 1), (-1, 2), (6, 1), (2, 2), (1, np.inf), (3, 4), (0, 1), (0, 1), (0, 1), (3, 4)])
    asked = np.column_stack([ij, np.full(len(ij), -7.0), np.full(len(ij), t)])
    asked[8:11, 3] = (np.nan, np.inf, -np.inf)
    out, info, status = screen_track(asked, c["T0"], c["T1"], eph=c["eph"])
    assert status.tolist() == [0, 9, 9, 9, 9, 9, 9, 0, 9, 9, 9, 0]
    bad = status == 9
    assert np.isnan(out[bad, 2:]).all() and (info[bad] == [-1, 0]).all() and np.array_equal(out[:, :2], asked[:, :2], equal_nan=True)
    alone = screen_track(asked[~bad], c["T0"], c["T1"], eph=c["eph"])
    assert out[~bad].tobytes() == alone[0].tobytes() and info[~bad].tobytes() == alone[1].tobytes() and np.isfinite(out[~bad, 2:]).all()
    assert out[7].tobytes() == out[11].tobytes()
    cc, cref = E.cross_case(6, 9, 66)
    ij = np.array([(5, 8), (0, 9), (6, 0), (2, 2), (-1, 3), (0, 6)])
    asked = np.column_stack([ij, np.full(6, -7.0), np.full(6, 0.5 * (cc["T0"] + cc["T1"]))])
    out, info, status = screen_track(asked, cc["T0"], cc["T1"], eph=cc["eph"], cat_eph=cc["cat_eph"])
    assert status.tolist() == [0, 9, 9, 0, 9, 0]                     # (against a catalogue i == j is a pair like any other)
    want = T.track_rows(asked, cref, 6, 9)
    assert info.tolist() == want["info"].tolist()


def test_c_abi_defines_every_byte_and_refuses_bad_arguments():
    from mpconstellation_amd import _ffi
    c, ref, listed, ev = full(130, 3.0)
    lib, ctx = _ffi.load(), _ffi.context(0)
    t = 0.5 * (c["T0"] + c["T1"])
    pairs = np.array([(0, 1, -7.0, t), (2, 2, -7.0, t), (np.nan, 0, -7.0, t), (3, 4, -7.0, np.nan), (1, 5, -7.0, t), (1, 5, -7.0, c["T1"] + 5.0)])
    n = len(pairs)
    eph = _ffi.as_f64(c["eph"])

    def call(poison, n=n, shift=0.0, out=True, status=True, info=True, T1=c["T1"], M=130, S=6):
        o = np.frombuffer(bytes([poison]) * (len(pairs) * 32), dtype=np.float64).copy().reshape(-1, 4)
        inf = np.frombuffer(bytes([poison]) * (len(pairs) * 8), dtype=np.int32).copy().reshape(-1, 2)
        st = np.frombuffer(bytes([poison]) * (len(pairs) * 4), dtype=np.int32).copy()
        rc = lib.mpcx_conjunction_track(ctx, n, _ffi.dptr(pairs), S, 0, M, _ffi.dptr(eph), None, c["T0"], T1, shift, _ffi.dptr(o) if out else None,
                                        _ffi.iptr(inf) if info else None, _ffi.iptr(st) if status else None)
        return rc, o, inf, st
    a, b = call(0xA5), call(0x5A)
    assert a[0] == 0 and b[0] == 0 and all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:]))      # nothing of the poison is left
    rc, o, inf, st = a
    assert st.tolist() == [0, 9, 9, 9, 0, 0] and np.array_equal(o[:, :2], pairs[:, :2], equal_nan=True)
    assert np.isnan(o[1:4, 2:]).all() and (inf[1:4] == [-1, 0]).all() and np.isfinite(o[[0, 4, 5], 2:]).all() and (inf[[0, 4, 5], 0] >= 0).all()
    assert inf[5, 0] == ref[(1, 5)].interval[-1]                     # a time after T1: the pair's last event
    a, b = call(0xA5, shift=1.0), call(0x5A, shift=1.0)              # a limit that cuts every good row: (+inf, NaN), (-1, 0), defined too
    assert a[0] == 0 and all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:]))
    assert np.isposinf(a[1][[0, 4, 5], 2]).all() and np.isnan(a[1][[0, 4, 5], 3]).all() and (a[2] == [-1, 0]).all() and a[3].tolist() == st.tolist()
    bare = call(0xA5, info=False)                                    # info may be NULL: the same out and status, info untouched
    assert bare[0] == 0 and bare[1].tobytes() == o.tobytes() and bare[3].tobytes() == st.tobytes() and (bare[2].view(np.uint8) == 0xA5).all()
    untouched = call(0xA5, n=0)
    assert untouched[0] == 0 and all((x.view(np.uint8) == 0xA5).all() for x in untouched[1:])      # n = 0: a successful no-op
    for bad in (dict(n=-1), dict(S=0), dict(M=1), dict(T1=c["T0"]), dict(shift=np.nan), dict(out=False), dict(status=False)):
        got = call(0xA5, **bad)
        assert got[0] == -2, bad
        assert b"conjunction_track" in lib.mpcx_last_error(ctx)
        assert all((x.view(np.uint8) == 0xA5).all() for x in got[1:])
    w = lib.mpcx_conjunction_track_workspace_bytes
    assert w(0, 0, 4) == 0 and w(2, 3, 4) == lib.mpcx_conjunction_pairs_workspace_bytes(2, 3, 4) > w(2, 0, 4) >= 2 * 6 * 4 * 8
