"""Every close approach of listed pairs on the device (csrc/conjunction.hip: events_kernel, one wave per pair, chunks of 64
consecutive intervals with the neighbour test across lanes and across chunks) against
  the numpy restatement (conjunction_events_reference.py): the same counts, intervals and edge flags, distance within 1e-6 m +
    1e-12 d and time within 1e-6 s -- the tolerances test_conjunction_gpu.py holds the screens to against the same restatement.
    Comparing event SETS is sound because every event's q is at least 1e-9 relative away from its present neighbours' in the
    restatement (asserted; the smallest gap on these scenes is 1.9e-7), far above the rounding of q;
  screen_pairs, byte for byte: a pair's smallest event (the earliest of equal ones) carries screen_pairs' distance and time;
  itself, byte for byte: the list permuted, (i, j) swapped, from ephemerides and from trajectories, on two contexts.
Grids on 6 satellites: M = 2 one interval, 17 fewer intervals than lanes, 65 exactly one chunk, 66 a second chunk of one interval,
130 a third chunk of one interval; the three-revolution scenes have events in intervals 63, 64 and 128 (asserted), the last and the
first lane of a chunk, so the carry between chunks is exercised in both directions."""
import functools

import numpy as np
import pytest

import conjunction_reference as R
import conjunction_cross_reference as X
import conjunction_events_reference as E

pytestmark = pytest.mark.gpu

ALL = 1e12                                                           # metres: every pair with a valid interval is listed
SCENES = [(65, 3.0), (66, 3.0), (130, 3.0), (2, 1.0), (17, 1.0)]     # (M, revolutions)
EDGE_LANES = {65: {63}, 66: {64}, 130: {64, 128}}                    # intervals the restatement must hold events in
THR = 2.0e6
S6 = np.array([(i, j) for i in range(6) for j in range(i + 1, 6)], dtype=np.float64)
S6X9 = np.array([(i, j) for i in range(6) for j in range(9)], dtype=np.float64)


def restated(M, orbits):
    return E.case(6, M, n=120, orbits=3.0) if orbits == 3.0 else E.case(6, M)


def rows(ij):
    """(n, 2) index pairs -> an (n, 4) list whose last two columns must not be read"""
    return np.column_stack([ij, np.full((len(ij), 2), -7.0)])


def bits(ev):
    return (ev.events.tobytes(), ev.row.tobytes(), ev.interval.tobytes(), ev.edge.tobytes(), ev.count.tobytes(), ev.truncated.tobytes(),
            ev.status.tobytes())


def of_row(ev, k):
    """(events, interval, edge) of list row k"""
    at = ev.row == k
    return ev.events[at], ev.interval[at], ev.edge[at]


def assert_matches_restatement(ev, listed, ref):
    """ev: the device's events of the list `listed` (n, >= 2); ref {(i, j): PairEvents}; a pair the restatement does not know has
    no valid interval"""
    worst_d = worst_t = 0.0
    for k, (i, j) in enumerate(listed[:, :2].astype(int).tolist()):
        e, m, edge = of_row(ev, k)
        p = ref.get((i, j)) or ref.get((j, i))
        if p is None:
            assert ev.count[k] == 0 and len(e) == 0
            continue
        assert ev.count[k] == p.count and m.tolist() == p.interval.tolist() and edge.tolist() == p.edge.tolist(), (i, j, m, p.interval, edge, p.edge)
        assert np.array_equal(e[:, :2], np.tile(listed[k, :2], (len(e), 1)))
        if len(e):
            worst_d = max(worst_d, float((np.abs(e[:, 2] - p.d) / (1e-6 + 1e-12 * p.d)).max()))
            worst_t = max(worst_t, float(np.abs(e[:, 3] - p.t).max()))
    print(f"    worst |d - d_ref| / (1e-6 m + 1e-12 d) {worst_d:.3e}, worst |t - t_ref| {worst_t:.3e} s")
    assert worst_d <= 1.0 and worst_t <= 1e-6


def assert_smallest_is_screen_pairs(ev, out):
    """per list row the event with the smallest distance, the earliest of equal ones, has screen_pairs' bytes"""
    for k in range(len(out)):
        e, _, _ = of_row(ev, k)
        if len(e) == 0:
            assert np.isposinf(out[k, 2]) and np.isnan(out[k, 3]) and ev.count[k] == 0
            continue
        best = int(np.argmin(e[:, 2]))                               # (the first of equal ones)
        assert e[best, 2:].tobytes() == out[k, 2:].tobytes(), (k, e[best], out[k])


@functools.lru_cache(maxsize=None)
def full(M, orbits):
    """the screen's list of every pair on the restated ephemeris and ALL its events on the device -> (case, restated events, list, events)"""
    from mpconstellation_amd import screen, screen_events
    c, ref = restated(M, orbits)
    r = screen(c["eph"], c["T0"], c["T1"], threshold=ALL)
    assert len(r.pairs) == 15
    most = max(p.count for p in ref.values())
    return c, ref, r.pairs, screen_events(r, c["T0"], c["T1"], max_events=most, eph=c["eph"])


@pytest.mark.parametrize("M,orbits", SCENES)
def test_against_the_restatement(M, orbits):
    c, ref, listed, ev = full(M, orbits)
    gap = E.smallest_gap(ref)
    print(f"M {M}: counts {sorted(p.count for p in ref.values())}, smallest relative gap of an event's q to a neighbour's {gap:.3e}")
    assert gap >= E.GAP
    if orbits == 3.0:
        assert max(p.count for p in ref.values()) == 7
        held = {int(m) for p in ref.values() for m in p.interval}
        assert EDGE_LANES[M] <= held, (M, sorted(held))              # events on the last / first lane of a chunk: not vacuous
    assert (ev.status == 0).all() and not ev.truncated.any() and ev.eph_status is None and ev.cat_status is None
    assert_matches_restatement(ev, listed, ref)
    assert np.array_equal(ev.row, np.sort(ev.row)) and all(np.all(np.diff(of_row(ev, k)[0][:, 3]) > 0) for k in range(15))


@pytest.mark.parametrize("M,orbits", SCENES)
def test_the_smallest_event_has_screen_pairs_bytes_in_every_form(M, orbits):
    from mpconstellation_amd import common_clock, screen, screen_events, screen_pairs
    c, ref, listed, ev = full(M, orbits)
    grid, E_max = (c["T0"], c["T1"]), ev.max_events
    out, status = screen_pairs(listed, *grid, eph=c["eph"])
    assert out.tobytes() == listed.tobytes()
    assert_smallest_is_screen_pairs(ev, out)
    # the list permuted: every pair's events move with it
    perm = np.random.default_rng(M).permutation(15)
    evp = screen_events(listed[perm], *grid, max_events=E_max, eph=c["eph"])
    assert evp.count.tobytes() == ev.count[perm].tobytes()
    for k, src in enumerate(perm):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(of_row(evp, k), of_row(ev, src)))
    # (j, i): the same operations on the same operands
    swapped = np.ascontiguousarray(listed[:, [1, 0, 2, 3]])
    evs = screen_events(swapped, *grid, max_events=E_max, eph=c["eph"])
    assert evs.events[:, [1, 0, 2, 3]].tobytes() == ev.events.tobytes() and bits(evs)[1:] == bits(ev)[1:]
    # two contexts
    assert bits(screen_events(listed, *grid, max_events=E_max, eph=c["eph"], devices=[0, 0])) == bits(ev)
    # from trajectories: the device's own ephemeris, never off the device; the same bits as common_clock followed by the call
    traj = dict(Y=c["Y"], units=c["units"], span=c["span"], M=M)
    rt = screen(T0=c["T0"], T1=c["T1"], threshold=ALL, **traj)
    evt = screen_events(rt, *grid, max_events=E_max, **traj)
    assert len(rt.pairs) == 15 and evt.eph_status.tolist() == [0] * 6 and evt.cat_status is None and (evt.status == 0).all()
    outt = screen_pairs(rt, *grid, **traj)[0]
    assert outt.tobytes() == rt.pairs.tobytes()
    assert_smallest_is_screen_pairs(evt, outt)
    assert bits(screen_events(rt, *grid, max_events=E_max, eph=common_clock(c["Y"], c["units"], c["span"], M, *grid))) == bits(evt)
    evt2 = screen_events(rt, *grid, max_events=E_max, devices=[0, 0], **traj)
    assert bits(evt2) == bits(evt) and evt2.eph_status.tolist() == [0] * 6
    assert_matches_restatement(evt, rt.pairs, ref)                   # (the device's ephemeris is the restated one to rounding)


@pytest.mark.parametrize("M", [65, 66, 130])
def test_threshold_keeps_the_events_at_or_below_it(M):
    from mpconstellation_amd import screen_events
    c, ref, listed, ev = full(M, 3.0)
    evt = screen_events(listed, c["T0"], c["T1"], threshold=THR, max_events=ev.max_events, eph=c["eph"])
    keep = ev.events[:, 2] <= THR
    assert 0 < keep.sum() < len(keep)
    assert evt.events.tobytes() == ev.events[keep].tobytes() and evt.row.tobytes() == ev.row[keep].tobytes()
    assert evt.interval.tobytes() == ev.interval[keep].tobytes() and evt.edge.tobytes() == ev.edge[keep].tobytes()
    assert evt.count.tolist() == np.bincount(ev.row[keep], minlength=15).tolist() and (evt.status == 0).all()
    if M == 130:
        assert sum((p.d <= THR).sum() >= 6 for p in ref.values()) >= 1 and evt.count.max() >= 3
    for thr in (None, 0.0, -1.0):                                    # no threshold: every event
        assert bits(screen_events(listed, c["T0"], c["T1"], threshold=thr, max_events=ev.max_events, eph=c["eph"])) == bits(ev)


@pytest.mark.parametrize("M", [66, 130])
def test_truncation_keeps_the_earliest_and_counts_them_all(M):
    from mpconstellation_amd import screen_events
    c, ref, listed, ev = full(M, 3.0)
    cut = screen_events(listed, c["T0"], c["T1"], max_events=2, eph=c["eph"])
    assert cut.count.tobytes() == ev.count.tobytes() and cut.truncated.tolist() == (ev.count > 2).tolist() and cut.truncated.any()
    assert len(cut.events) == int(np.minimum(ev.count, 2).sum())
    for k in range(15):
        assert all(a.tobytes() == b[:2].tobytes() for a, b in zip(of_row(cut, k), of_row(ev, k)))


@pytest.mark.parametrize("M", [17, 66])
def test_catalogue_form(M):
    from mpconstellation_amd import screen_against, screen_events, screen_pairs
    c, ref = E.cross_case(6, 9, M)
    grid = (c["T0"], c["T1"])
    gap = E.smallest_gap(ref)
    most = max(p.count for p in ref.values())
    print(f"6 x 9, M {M}: largest count {most}, smallest gap {gap:.3e}")
    assert gap >= E.GAP
    r = screen_against(c["eph"], c["cat_eph"], *grid, threshold=ALL)
    assert len(r.pairs) == 54
    ev = screen_events(r, *grid, max_events=most, eph=c["eph"], cat_eph=c["cat_eph"])
    assert (ev.status == 0).all() and not ev.truncated.any()
    for k, (i, j) in enumerate(r.pairs[:, :2].astype(int).tolist()):          # (against a catalogue (i, j) is not (j, i))
        p = ref[(i, j)]
        e, m, edge = of_row(ev, k)
        assert m.tolist() == p.interval.tolist() and edge.tolist() == p.edge.tolist() and ev.count[k] == p.count
        assert (np.abs(e[:, 2] - p.d) <= 1e-6 + 1e-12 * p.d).all() and (np.abs(e[:, 3] - p.t) <= 1e-6).all()
    out, _ = screen_pairs(r, *grid, eph=c["eph"], cat_eph=c["cat_eph"])
    assert out.tobytes() == r.pairs.tobytes()
    assert_smallest_is_screen_pairs(ev, out)
    perm = np.random.default_rng(M).permutation(54)
    evp = screen_events(r.pairs[perm], *grid, max_events=most, eph=c["eph"], cat_eph=c["cat_eph"], devices=[0, 0])
    for k, src in enumerate(perm):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(of_row(evp, k), of_row(ev, src)))
    traj = dict(M=M, **c["sat"], **c["cat"])
    rt = screen_against(T0=c["T0"], T1=c["T1"], threshold=ALL, **traj)
    evt = screen_events(rt, *grid, max_events=most, **traj)
    assert evt.eph_status.tolist() == [0] * 6 and evt.cat_status.tolist() == [0] * 9 and (evt.status == 0).all()
    assert_smallest_is_screen_pairs(evt, screen_pairs(rt, *grid, **traj)[0])
    assert bits(screen_events(rt, *grid, max_events=most, devices=[0, 0, 0], **traj)) == bits(evt)
    assert evt.interval.tolist() == ev.interval.tolist() and evt.edge.tolist() == ev.edge.tolist()


def ragged(M):
    """6 satellites and 9 objects with n = 40 nodes over one revolution: spans that end or begin inside the grid, two satellites that
    are never on the grid together, a satellite and an object with a single node in use, an object that is never on the grid, and
    node counts below n with garbage behind them -> (sat, cat, T0, T1)"""
    orb = R.random_orbits(15, seed=77 + M)
    T0, T1 = 0.0, 2 * np.pi / R.orbit_rate(orb).max()
    span = np.tile([T0 - 1.0, T1 + 1.0], (15, 1))
    span[1] = (T0 - 1.0, 0.4 * T1)
    span[2] = (0.6 * T1, T1 + 1.0)                                   # never on the grid together with satellite 1
    span[4] = (0.3 * T1, 0.7 * T1)
    span[6 + 2] = (T0 - 1.0, 0.35 * T1)
    span[6 + 5] = (0.65 * T1, T1 + 1.0)
    span[6 + 7] = (T1 + 10.0, T1 + 500.0)                            # an object that is never on the grid
    Y, units, span = R.trajectories(orb, 40, span)
    ns = np.full(15, 40, dtype=np.int32)
    ns[3] = 1; ns[6 + 4] = 1                                         # a single node: no ephemeris, status 9
    ns[5] = 23; ns[6 + 1] = 31
    for s in (5, 6 + 1):                                             # the trajectory on its own count, garbage past it
        Yk, _, _ = R.trajectories({k: v[s:s + 1] for k, v in orb.items()}, int(ns[s]), span[s])
        Y[s] = 1e300; Y[s, :, :ns[s]] = Yk[0]
    sat = dict(Y=Y[:6], units=units[:6], span=span[:6], ns=ns[:6])
    cat = dict(cat_Y=Y[6:], cat_units=units[6:], cat_span=span[6:], cat_ns=ns[6:])
    return sat, cat, T0, T1


@pytest.mark.parametrize("M", [66, 130])
def test_ragged_spans_and_counts(M):
    from mpconstellation_amd import screen_events
    sat, cat, T0, T1 = ragged(M)
    eph, st = R.ephemeris(sat["Y"], sat["units"], sat["span"], M, T0, T1, sat["ns"])
    ceph, cst = R.ephemeris(cat["cat_Y"], cat["cat_units"], cat["cat_span"], M, T0, T1, cat["cat_ns"])
    assert st.tolist() == [0, 0, 0, 9, 0, 0] and cst.tolist() == [0, 0, 0, 0, 9, 0, 0, 0, 0]
    tg, _ = R.grid(M, T0, T1)
    for listed, ref, kw in ((rows(S6), E.all_pairs(eph, T0, T1), {}), (rows(S6X9), E.against(eph, ceph, T0, T1), cat)):
        assert E.smallest_gap(ref) >= E.GAP
        most = max(p.count for p in ref.values())
        ev = screen_events(listed, T0, T1, max_events=most, M=M, **sat, **kw)
        assert (ev.status == 0).all() and ev.eph_status.tolist() == st.tolist()
        assert ev.cat_status is None if not kw else ev.cat_status.tolist() == cst.tolist()
        assert_matches_restatement(ev, listed, ref)
        # a pair whose common span ends inside the grid while the two are closing: an edge event at its last valid instant
        closing = [(k, p) for k, p in ref.items() if p.count and p.edge[-1] and p.interval[-1] < M - 2 and p.t[-1] == tg[p.interval[-1] + 1]]
        assert closing, "no pair of the scene is still closing where its span ends"
        for (i, j), p in closing:
            k = int(np.flatnonzero((listed[:, 0] == i) & (listed[:, 1] == j))[0])
            e, m, edge = of_row(ev, k)
            assert edge[-1] and m[-1] == p.interval[-1] and abs(e[-1, 3] - tg[m[-1] + 1]) <= 1e-6
        never = [k for k, (i, j) in enumerate(listed[:, :2].astype(int).tolist()) if not np.isfinite(ref[(i, j)].q).any()]
        assert never and (ev.count[never] == 0).all() and (ev.status[never] == 0).all()
        if not kw:
            assert ref[(1, 2)].count == 0 and all(ref[k].count == 0 for k in ref if 3 in k)      # never together; the single node
        assert bits(screen_events(listed, T0, T1, max_events=most, M=M, devices=[0, 0], **sat, **kw)) == bits(ev)


def test_bad_rows_are_reported_and_leave_their_neighbours_alone():
    from mpconstellation_amd import screen_events
    c, ref, listed, ev = full(130, 3.0)
    want = {(int(i), int(j)): k for k, (i, j) in enumerate(listed[:, :2])}
    ij = np.array([(0, 1), (np.nan, 1), (0.5, 1), (-1, 2), (6, 1), (2, 2), (1, np.inf), (3, 4)])
    got = screen_events(rows(ij), c["T0"], c["T1"], max_events=ev.max_events, eph=c["eph"])
    assert got.status.tolist() == [0, 9, 9, 9, 9, 9, 9, 0] and got.count[1:7].tolist() == [0] * 6 and set(got.row.tolist()) == {0, 7}
    for k, key in ((0, (0, 1)), (7, (3, 4))):
        assert all(a[:, -2:].tobytes() == b[:, -2:].tobytes() if a.ndim == 2 else a.tobytes() == b.tobytes()
                   for a, b in zip(of_row(got, k), of_row(ev, want[key])))
    cc, cref = E.cross_case(6, 9, 66)
    ij = np.array([(5, 8), (0, 9), (6, 0), (2, 2), (-1, 3), (0, 6)])
    got = screen_events(rows(ij), cc["T0"], cc["T1"], eph=cc["eph"], cat_eph=cc["cat_eph"])
    assert got.status.tolist() == [0, 9, 9, 0, 9, 0] and got.count[[1, 2, 4]].tolist() == [0, 0, 0]
    for k in (0, 3, 5):                                              # (against a catalogue i == j is a pair like any other)
        assert of_row(got, k)[1].tolist() == cref[tuple(ij[k].astype(int))].interval.tolist()


def test_c_abi_defines_every_byte_and_refuses_bad_arguments():
    from mpconstellation_amd import _ffi
    c, ref, listed, ev = full(130, 3.0)
    lib, ctx = _ffi.load(), _ffi.context(0)
    ij = np.array([(0, 1), (2, 2), (np.nan, 0), (3, 4), (1, 5)])
    pairs, n, E_max = rows(ij), 5, 9                                 # more slots than any pair has events, and a cut-off call below
    eph = _ffi.as_f64(c["eph"])

    def call(poison, E_slots, n=n, thr=0.0, events=True, T1=c["T1"], M=130, S=6):
        slots = max(E_slots, 1)                                      # (room for the calls that must be refused, too)
        ev_b = np.frombuffer(bytes([poison]) * (5 * slots * 32), dtype=np.float64).copy().reshape(5, slots, 4)
        info = np.frombuffer(bytes([poison]) * (5 * slots * 8), dtype=np.int32).copy().reshape(5, slots, 2)
        count = np.frombuffer(bytes([poison]) * 20, dtype=np.int32).copy()
        status = np.frombuffer(bytes([poison]) * 20, dtype=np.int32).copy()
        rc = lib.mpcx_conjunction_events(ctx, n, _ffi.dptr(pairs), S, 0, M, _ffi.dptr(eph), None, c["T0"], T1, thr, E_slots,
                                         _ffi.dptr(ev_b) if events else None, _ffi.iptr(info), _ffi.iptr(count), _ffi.iptr(status))
        return rc, ev_b, info, count, status
    for E_slots in (E_max, 2):
        a, b = call(0xA5, E_slots), call(0x5A, E_slots)
        assert a[0] == 0 and b[0] == 0 and all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:]))     # nothing of the poison is left
        rc, ev_b, info, count, status = a
        assert status.tolist() == [0, 9, 9, 0, 0] and count[[1, 2]].tolist() == [0, 0]
        assert np.array_equal(ev_b[:, :, :2], np.broadcast_to(ij[:, None, :], (5, E_slots, 2)), equal_nan=True)
        for k in range(5):
            kept = min(int(count[k]), E_slots)
            assert np.isfinite(ev_b[k, :kept, 2:]).all() and np.isnan(ev_b[k, kept:, 2:]).all()
            assert (info[k, :kept, 0] >= 0).all() and (info[k, kept:] == [-1, 0]).all()
    untouched = call(0xA5, 3, n=0)
    assert untouched[0] == 0 and all((x.view(np.uint8) == 0xA5).all() for x in untouched[1:])      # n = 0: a successful no-op
    for bad in (dict(n=-1), dict(S=0), dict(M=1), dict(T1=c["T0"]), dict(E_slots=0), dict(E_slots=-3), dict(thr=np.nan), dict(events=False)):
        assert call(0xA5, **{"E_slots": 3, **bad})[0] == -2, bad
        assert b"conjunction_events" in lib.mpcx_last_error(ctx)
    w = lib.mpcx_conjunction_events_workspace_bytes
    assert w(0, 0, 4) == 0 and w(2, 3, 4) == lib.mpcx_conjunction_pairs_workspace_bytes(2, 3, 4) > w(2, 0, 4) >= 2 * 6 * 4 * 8


# ---- downstream: repeated (i, j) with different times are independent rows of every call that takes a pairs list
@functools.lru_cache(maxsize=None)
def downstream():
    """the three-revolution scene's events at or below 2000 km of four listed pairs -- the three with the most such events and one
    with none --, and what the downstream calls need beside them: zero thrust, the satellites' constants, and a covariance (500 km
    in position: the events are hundreds of km apart, and a probability that underflows would make the product vacuous)"""
    from mpconstellation_amd import screen_events
    from mpconstellation_amd.satellite_scale import SatelliteScale
    c, ref, listed, _ = full(130, 3.0)
    below = np.array([(ref[(int(i), int(j))].d <= THR).sum() for i, j in listed[:, :2]])
    assert (below == 0).any() and np.sort(below)[-3] >= 3
    some = np.sort(np.concatenate([np.argsort(-below, kind="stable")[:3], np.flatnonzero(below == 0)[:1]]))
    ev = screen_events(listed[some], c["T0"], c["T1"], threshold=THR, eph=c["eph"])
    consts = np.stack([SatelliteScale(x=np.array([L, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])).get_normalized_constants().as_vector() for L in c["units"][:, 0]])
    P = np.ascontiguousarray(np.broadcast_to(np.diag([2.5e11] * 3 + [1.0] * 3), (6, 120, 6, 6)))
    return c, ev, consts, P, np.zeros((6, 3, 120))


def test_collision_probability_and_avoidance_take_the_events_row_by_row():
    from mpconstellation_amd import avoidance, collision_probability, cumulative_probability
    c, ev, consts, P, U = downstream()
    side = (c["Y"], c["units"], c["span"])
    n_ev = len(ev.events)
    assert n_ev >= 8 and ev.count.max() >= 3
    col = collision_probability(ev.events, 5.0e4, *side, P)
    one = [collision_probability(ev.events[k:k + 1], 5.0e4, *side, P) for k in range(n_ev)]
    assert (col.status == 0).all() and (col.pc > 0.0).all() and (col.pc < 1.0).all()
    for name in ("pc", "miss", "speed", "sigma", "mahalanobis", "status"):
        assert getattr(col, name).tobytes() == np.concatenate([getattr(r, name) for r in one]).tobytes(), name
    cum = cumulative_probability(ev, col.pc)
    want = np.array([1.0 - np.prod(1.0 - col.pc[ev.row == k]) for k in range(4)])
    print(f"pc {col.pc.min():.3e} .. {col.pc.max():.3e}; cumulative {cum.min():.3e} .. {cum.max():.3e}")
    # the plain product rounds 1 - p and the difference from 1: an absolute error of a few eps, whatever the size of the result
    assert cum.shape == (4,) and (np.abs(cum - want) <= 16 * np.finfo(np.float64).eps).all() and (cum[ev.count == 0] == 0.0).all()
    assert (ev.count == 0).sum() == 1
    assert (cum[ev.count > 1] > np.array([col.pc[ev.row == k].max() for k in np.flatnonzero(ev.count > 1)])).all()
    assert cumulative_probability(ev, col).tobytes() == cum.tobytes()
    av = avoidance(ev.events, 2.5e6, c["Y"], U, c["units"], c["span"], consts)
    ones = [avoidance(ev.events[k:k + 1], 2.5e6, c["Y"], U, c["units"], c["span"], consts) for k in range(n_ev)]
    assert (av.status == 0).all() and np.abs(av.du).max() > 0.0
    assert av.out.tobytes() == np.concatenate([r.out for r in ones]).tobytes()
    assert av.du.tobytes() == np.concatenate([r.du for r in ones]).tobytes()


def test_avoidance_joint_opens_all_events_of_one_pair():
    """existing code on a new kind of list: two or more rows of the SAME pair at different times, one mover"""
    from mpconstellation_amd import avoidance_joint, _ffi
    c, ev, consts, P, U = downstream()
    k = int(np.argmax(ev.count))
    mine = ev.events[ev.row == k]
    assert len(mine) >= 2 and len(mine) <= _ffi.AJ_MAX_ROWS
    mover, target, tol = int(mine[0, 0]), 1.05 * float(mine[:, 2].max()), _ffi.AJ_DEFAULT_TOL
    res = avoidance_joint(mine, target, c["Y"], U, c["units"], c["span"], consts, who="i", hold_terminal=False, tol=tol)
    print(f"pair {mine[0, :2]}, {len(mine)} events at {mine[:, 3]} s, d0 {res.d0}, margin {res.margin}, target {target}, status {res.status.tolist()}, "
          f"rows {res.n_rows.tolist()}, iterations {res.iters.tolist()}, residual {res.residual.tolist()}")
    assert res.status[mover] == 0 and (res.row_status == 0).all() and res.n_rows[mover] == len(mine)
    assert (res.margin >= target * (1.0 - tol)).all()                # (the rows' residual is in units of the target: include/mpcx.h)


def test_constellation_mpc_encounters():
    """Three satellites, one update over a horizon of two time units: ConstellationMPC.encounters lists the plan's pairs and returns,
    bit for bit, what the module-level calls return on the plan -- screen, screen_events at the same threshold, and with P0 and a
    radius the covariance along the plan, one probability per event and cumulative_probability per listed pair"""
    from mpconstellation_amd import Satellite, ConstellationMPC, conjunction as cj
    from mpconstellation_amd.constellation import constellation_states
    st = constellation_states(3)
    mpc = ConstellationMPC([Satellite(s[:3].copy(), s[3:6].copy(), float(s[6])) for s in st], base_res=30, tf_horizon=2, tf_interval=1, r_des=1.5)
    mpc.update()
    (w,) = mpc._screen_windows("plan", samples_per_node=4)
    thr = 1e9                                                        # every pair, every event
    scr, ev = mpc.encounters(thr, max_events=8)
    scr2 = cj.screen(threshold=thr, **w)
    ev2 = cj.screen_events(scr2, threshold=thr, max_events=8, **w)
    print("pairs", scr.pairs[:, :2].tolist(), "events per pair", ev.count.tolist(), "edge", ev.edge.tolist())
    assert len(scr.pairs) == 3 and scr.pairs.tobytes() == scr2.pairs.tobytes() and bits(ev) == bits(ev2)
    assert (ev.status == 0).all() and (ev.count >= 1).all() and ev.eph_status.tolist() == [0, 0, 0]
    assert_smallest_is_screen_pairs(ev, scr.pairs)
    P0 = np.diag([100.0 ** 2] * 3 + [0.1 ** 2] * 3)
    scr3, ev3, col, cum = mpc.encounters(thr, P0, 5.0, q=1e-8, max_events=8)
    P = cj.covariance(w["Y"], w["units"], w["span"], mpc.consts, P0, U=mpc._plan[1], ns=w["ns"], q=1e-8)
    col2 = cj.collision_probability(ev2.events, 5.0, w["Y"], w["units"], w["span"], P, ns=w["ns"])
    assert bits(ev3) == bits(ev) and col.pc.tobytes() == col2.pc.tobytes() and col.status.tobytes() == col2.status.tobytes()
    assert cum.shape == (3,) and cum.tobytes() == cj.cumulative_probability(ev2, col2.pc).tobytes()
    with pytest.raises(ValueError):
        mpc.encounters(thr, P0=P0)
    with pytest.raises(ValueError):
        mpc.encounters(thr, catalogue=(1, 2, 3, 4, 5))
