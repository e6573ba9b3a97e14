"""Conjunction screening on the device (csrc/conjunction.hip) against its numpy restatement (conjunction_reference.py).

Tolerances, from the arithmetic: positions of 7e6 m times 2.2e-16 times about 100 operations is about 2e-7 m, so
|dmin - restated| <= 1e-6 m + 1e-12 dmin; the partner is identical (the inputs have no ties, asserted); a 1e-9 m rounding over a
relative speed of at least 1 m/s (asserted) is far below 1e-6 s, the bound on tca.
Shapes: the kernel's row tile is 256, its column tile 16, its LDS chunk 32 intervals -- one less, one more, not a multiple."""
import ctypes as C

import numpy as np
import pytest

import conjunction_reference as R

pytestmark = pytest.mark.gpu

SHAPES = [2, 3, 15, 17, 65, 255, 257, 300]
GRIDS = [2, 3, 17, 130]


def close(res, ref):
    assert np.array_equal(res.partner, ref.partner)
    fin = ref.partner >= 0
    assert (np.abs(res.dmin[fin] - ref.dmin[fin]) <= 1e-6 + 1e-12 * ref.dmin[fin]).all(), np.abs(res.dmin[fin] - ref.dmin[fin]).max()
    assert (np.abs(res.tca[fin] - ref.tca[fin]) <= 1e-6).all(), np.abs(res.tca[fin] - ref.tca[fin]).max()
    assert np.isposinf(res.dmin[~fin]).all() and np.isnan(res.tca[~fin]).all()


def assert_no_ties_and_moving(c):
    """what the tolerances above assume of a generated case: every row's nearest partner is nearer than the next one by far more
    than the rounding, and every pair moves at >= 1 m/s relative to each other at every instant"""
    ref, eph = c["ref"], c["eph"]
    S = eph.shape[0]
    if S > 2:
        q = np.sort(np.sqrt(ref.Q), axis=1)
        assert (q[:, 1] - q[:, 0] > 1e-3).all()
    lo, hi = np.triu_indices(S, 1)
    w = eph[hi, 3:6, :] - eph[lo, 3:6, :]
    assert np.sqrt((w * w).sum(axis=1)).min() >= 1.0


def bits(r):
    return (r.dmin.tobytes(), r.partner.tobytes(), r.tca.tobytes(), r.pairs.tobytes(), r.n_pairs_total)


@pytest.mark.parametrize("M", GRIDS)
@pytest.mark.parametrize("S", SHAPES)
def test_against_the_restatement(S, M):
    from mpconstellation_amd import common_clock, screen
    c = R.case(S, M)
    assert_no_ties_and_moving(c)
    eph = common_clock(c["Y"], c["units"], c["span"], M, c["T0"], c["T1"])
    assert np.abs(eph - c["eph"]).max() <= 1e-6                      # metres and m/s: the same few operations on 7e6 m
    close(screen(eph, c["T0"], c["T1"]), c["ref"])                   # (its 1e-8 m away from the restated ephemeris is 1e-11 s at 1 km/s)
    close(screen(c["eph"], c["T0"], c["T1"]), c["ref"])              # the restated ephemeris in: the screen alone


@pytest.mark.parametrize("M", [33, 34])
def test_grid_at_the_lds_chunk(M):
    from mpconstellation_amd import screen
    c = R.case(65, M)
    assert_no_ties_and_moving(c)
    close(screen(c["eph"], c["T0"], c["T1"]), c["ref"])


def test_symmetry():
    """mutual nearest neighbours hold the same bits: both orderings of a pair run the same arithmetic"""
    from mpconstellation_amd import screen
    c = R.case(300, 130)
    r = screen(c["eph"], c["T0"], c["T1"])
    i = np.arange(300)
    mutual = r.partner[r.partner] == i
    assert mutual.sum() >= 2
    assert np.array_equal(r.dmin[mutual], r.dmin[r.partner[mutual]]) and np.array_equal(r.tca[mutual], r.tca[r.partner[mutual]])


def test_identical_trajectories_give_zero():
    from mpconstellation_amd import screen
    c = R.case(3, 17)
    Y = c["Y"].copy(); Y[2] = Y[0]
    units = c["units"].copy(); units[2] = units[0]
    r = screen(Y=Y, units=units, span=c["span"], M=17, T0=c["T0"], T1=c["T1"])
    assert r.dmin[0] == 0.0 and r.dmin[2] == 0.0


def test_span_that_misses_the_grid_and_partial_overlap():
    from mpconstellation_amd import common_clock, screen
    S, M, n = 17, 40, 30
    orb = R.random_orbits(S, seed=5)
    T0, T1 = 0.0, 3000.0
    span = np.tile([T0 - 1.0, T1 + 1.0], (S, 1))
    span[4] = (T1 + 100.0, T1 + 2000.0)                              # never on the grid
    span[7] = (1000.0, 2100.0); span[9] = (T0 - 500.0, 1500.0); span[11] = (1500.0, 1560.0)      # partly; 11 sees one instant only
    Y, units, span = R.trajectories(orb, n, span)
    eph_ref, _ = R.ephemeris(Y, units, span, M, T0, T1)
    ref = R.screen(eph_ref, T0, T1)
    eph, status = common_clock(Y, units, span, M, T0, T1, return_status=True)
    assert (status == 0).all() and np.array_equal(np.isnan(eph), np.isnan(eph_ref)) and np.isnan(eph[4]).all()
    r = screen(eph_ref, T0, T1)
    close(r, ref)
    assert r.partner[4] == -1 and np.isposinf(r.dmin[4]) and np.isnan(r.tca[4]) and not (r.partner == 4).any()
    assert r.partner[11] == -1                                       # one instant inside its span: no interval with two valid ends
    assert (np.delete(r.partner, [4, 11]) >= 0).all()
    close(screen(Y=Y, units=units, span=span, M=M, T0=T0, T1=T1), ref)


def test_ragged_counts_ignore_what_lies_past_them():
    from mpconstellation_amd import common_clock, screen
    c = R.case(17, 17)
    n, k = c["Y"].shape[2], 23
    orb = c["orb"]
    Yk, units, span = R.trajectories(orb, k, c["span"])
    Yg = np.full((17, 7, n), 1e300); Yg[:, :, :k] = Yk
    Yg[3, :, k:] = np.nan
    a = common_clock(Yk, units, span, 17, c["T0"], c["T1"])
    b = common_clock(Yg, units, span, 17, c["T0"], c["T1"], ns=np.full(17, k))
    assert np.array_equal(a, b) and not np.isnan(a).any()
    ra = screen(Y=Yk, units=units, span=span, M=17, T0=c["T0"], T1=c["T1"], threshold=1e9)
    rb = screen(Y=Yg, units=units, span=span, ns=np.full(17, k), M=17, T0=c["T0"], T1=c["T1"], threshold=1e9)
    assert bits(ra) == bits(rb)
    # different counts per satellite, against the restatement
    ns = np.array([k, n, 2, 9] * 4 + [k])
    Ym = np.full((17, 7, n), np.nan)
    for s in range(17):
        Ym[s, :, :ns[s]] = R.trajectories({key: v[s:s + 1] for key, v in orb.items()}, int(ns[s]), c["span"][s:s + 1])[0][0]
    eph_ref, _ = R.ephemeris(Ym, units, span, 17, c["T0"], c["T1"], ns=ns)
    eph = common_clock(Ym, units, span, 17, c["T0"], c["T1"], ns=ns)
    assert np.abs(eph - eph_ref).max() <= 1e-6


def test_bad_counts_and_spans_are_reported_per_satellite():
    from mpconstellation_amd import common_clock, screen
    c = R.case(3, 17)
    span = c["span"].copy(); span[2] = (5.0, 5.0)
    eph, status = common_clock(c["Y"], c["units"], span, 17, c["T0"], c["T1"], ns=[40, 1, 40], return_status=True)
    assert status.tolist() == [0, 9, 9] and np.isnan(eph[1:]).all() and not np.isnan(eph[0]).any()
    r = screen(Y=c["Y"], units=c["units"], span=span, ns=[40, 1, 40], M=17, T0=c["T0"], T1=c["T1"])
    assert r.status.tolist() == [0, 9, 9] and r.partner.tolist() == [-1, -1, -1]
    _, status = common_clock(c["Y"], c["units"], c["span"], 17, c["T0"], c["T1"], ns=[40, 41, 0], return_status=True)
    assert status.tolist() == [0, 9, 9]


def test_single_satellite():
    from mpconstellation_amd import screen
    c = R.case(2, 17)
    r = screen(c["eph"][:1], c["T0"], c["T1"], threshold=1e9)
    assert np.isposinf(r.dmin[0]) and r.partner[0] == -1 and np.isnan(r.tca[0]) and r.n_pairs_total == 0 and r.pairs.shape == (0, 4)


def test_pairs_list():
    from mpconstellation_amd import screen
    c = R.case(65, 130)
    ref = c["ref"]
    d = np.sort(ref.pairs[:, 2])
    thr = 0.5 * (d[9] + d[10])                                      # the ten closest of the 2080 pairs
    assert d[10] - d[9] > 1e-3
    want = ref.pairs_within(thr)
    r = screen(c["eph"], c["T0"], c["T1"], threshold=thr)
    assert r.n_pairs_total == 10 and np.array_equal(r.pairs[:, :2], want[:, :2])
    assert (np.abs(r.pairs[:, 2] - want[:, 2]) <= 1e-6 + 1e-12 * want[:, 2]).all() and (np.abs(r.pairs[:, 3] - want[:, 3]) <= 1e-6).all()
    cut = screen(c["eph"], c["T0"], c["T1"], threshold=thr, max_pairs=4)
    assert cut.n_pairs_total == 10 and cut.pairs.shape == (4, 4)
    full = {tuple(row) for row in r.pairs.tolist()}
    assert all(tuple(row) in full for row in cut.pairs.tolist())
    assert np.array_equal(cut.dmin, r.dmin) and np.array_equal(cut.partner, r.partner)
    none = screen(c["eph"], c["T0"], c["T1"])
    assert none.n_pairs_total == 0 and none.pairs.shape == (0, 4)


def test_fused_and_two_devices_hold_the_same_bits():
    from mpconstellation_amd import common_clock, screen
    c = R.case(300, 130)
    thr = np.sort(c["ref"].pairs[:, 2])[20]
    eph = common_clock(c["Y"], c["units"], c["span"], 130, c["T0"], c["T1"])
    two_step = screen(eph, c["T0"], c["T1"], threshold=thr)
    traj = dict(Y=c["Y"], units=c["units"], span=c["span"], M=130, T0=c["T0"], T1=c["T1"], threshold=thr)
    fused = screen(**traj)
    assert two_step.n_pairs_total >= 20 and bits(fused) == bits(two_step)
    assert bits(screen(eph, c["T0"], c["T1"], threshold=thr, devices=[0, 0])) == bits(two_step)
    assert bits(screen(devices=[0, 0, 0], **traj)) == bits(two_step)


def test_blocks_of_rows_hold_the_whole_call_s_bits():
    """mpcx_conjunction_screen for the whole square, and again for blocks of rows: a block's rows are read from the instant-major
    copy of the whole constellation at row0 + lane, which only the two-device test reached with row0 > 0.  S = 300 makes row 257
    the second workgroup's first lane and (299, 1) a block with one live lane; M = 34 is one interval past the 32-interval chunk."""
    from mpconstellation_amd import _ffi
    from mpconstellation_amd.conjunction import sort_pairs
    S, M = 300, 34
    c = R.case(S, M)
    lib, ctx = _ffi.load(), _ffi.context(0)
    eph = np.ascontiguousarray(c["eph"])
    npair = S * (S - 1) // 2

    def call(row0, nrows):
        d, p, t = np.empty(nrows), np.empty(nrows, dtype=np.int32), np.empty(nrows)
        pairs, n = np.zeros((npair, 4)), np.zeros(1, dtype=np.int64)
        assert lib.mpcx_conjunction_screen(ctx, S, M, _ffi.dptr(eph), c["T0"], c["T1"], row0, nrows, 1e9, npair, _ffi.dptr(d), _ffi.iptr(p),
                                           _ffi.dptr(t), _ffi.dptr(pairs), n.ctypes.data_as(_ffi._lp)) == 0
        assert n[0] <= npair
        return d, p, t, sort_pairs(pairs[:n[0]])
    wd, wp, wt, wpairs = call(0, S)
    assert len(wpairs) == npair and (wp >= 0).all()
    lists = []
    for row0, nrows in ((0, 257), (257, 43), (299, 1)):
        d, p, t, pairs = call(row0, nrows)
        rows = slice(row0, row0 + nrows)
        assert d.tobytes() == wd[rows].tobytes() and p.tobytes() == wp[rows].tobytes() and t.tobytes() == wt[rows].tobytes(), (row0, nrows)
        mine = wpairs[(wpairs[:, 0] >= row0) & (wpairs[:, 0] < row0 + nrows)]          # the pairs whose smaller index lies in the block
        assert pairs.tobytes() == mine.tobytes(), (row0, nrows)
        lists.append(pairs)
    assert sort_pairs(np.concatenate(lists)).tobytes() == wpairs.tobytes()


def test_c_abi_refuses_bad_arguments():
    from mpconstellation_amd import _ffi
    lib, ctx = _ffi.load(), _ffi.context(0)
    eph = np.zeros((2, 6, 4)); d = np.zeros(2); p = np.zeros(2, dtype=np.int32); t = np.zeros(2)
    pairs = np.zeros((4, 4)); n = np.zeros(1, dtype=np.int64)
    out = (_ffi.dptr(d), _ffi.iptr(p), _ffi.dptr(t), _ffi.dptr(pairs), n.ctypes.data_as(_ffi._lp))
    good = dict(S=2, M=4, T0=0.0, T1=1.0, row0=0, nrows=2, thr=1.0, max_pairs=4)
    for bad in (dict(M=1), dict(S=0), dict(T1=0.0), dict(T1=-1.0), dict(max_pairs=-1), dict(row0=1), dict(nrows=0)):
        a = {**good, **bad}
        rc = lib.mpcx_conjunction_screen(ctx, a["S"], a["M"], _ffi.dptr(eph), a["T0"], a["T1"], a["row0"], a["nrows"], a["thr"], a["max_pairs"], *out)
        assert rc == -2, bad
    Y = np.zeros((2, 7, 5)); u = np.ones((2, 2)); sp = np.array([[0.0, 1.0]] * 2); st = np.zeros(2, dtype=np.int32)
    for S, M, T1 in ((0, 4, 1.0), (2, 1, 1.0), (2, 4, 0.0)):
        assert lib.mpcx_ephemeris_batch(ctx, S, 5, None, _ffi.dptr(Y), _ffi.dptr(u), _ffi.dptr(sp), M, 0.0, T1, _ffi.dptr(eph), _ffi.iptr(st)) == -2
        assert lib.mpcx_conjunction_screen_traj(ctx, S, 5, None, _ffi.dptr(Y), _ffi.dptr(u), _ffi.dptr(sp), M, 0.0, T1, 0, 2, 0.0, 0, *out,
                                                _ffi.iptr(st)) == -2
    assert lib.mpcx_conjunction_workspace_bytes(0, 4) == 0 and lib.mpcx_conjunction_workspace_bytes(2, 4) > 0


def test_planted_conjunction_in_the_flown_segments():
    """64 satellites flown for two segments; one satellite's flown positions in the second segment are shifted so that it passes
    about 500 m from another: screen(what='flown', threshold_m=1000) reports exactly that pair, as the restatement does on the same
    arrays; the plans are screened too."""
    from mpconstellation_amd import Satellite, ConstellationMPC, conjunction as cj
    from mpconstellation_amd.constellation import constellation_states
    st = constellation_states(64)
    mpc = ConstellationMPC([Satellite(s[:3].copy(), s[3:6].copy(), float(s[6])) for s in st], base_res=30, tf_horizon=2, tf_interval=1,
                           r_des=1.5, sim_base_res=100)
    mpc.run_segments(tf=2, num_segments=2)
    a, b, k = 5, 40, 37
    y = mpc._seg_y[1]
    L = np.array([sc.units["length"] for sc in mpc.scales]); V = L / np.array([sc.units["time"] for sc in mpc.scales])
    w = y[b, 3:6, k] * V[b] - y[a, 3:6, k] * V[a]                   # relative velocity at the planted instant (m/s)
    e = np.cross(w, [0.0, 0.0, 1.0]); e /= np.linalg.norm(e)        # the miss vector: across the relative motion
    assert np.linalg.norm(w) >= 1.0
    y[a, 0:3, :] += ((y[b, 0:3, k] * L[b] - y[a, 0:3, k] * L[a] + 500.0 * e) / L[a])[:, None]
    windows = mpc._screen_windows("flown", samples_per_node=4)
    refs = []
    for wdw in windows:
        eph, _ = R.ephemeris(wdw["Y"], wdw["units"], wdw["span"], wdw["M"], wdw["T0"], wdw["T1"])
        rr = R.screen(eph, wdw["T0"], wdw["T1"])
        refs.append(cj.ConjunctionResult(rr.dmin, rr.partner, rr.tca, rr.pairs_within(1000.0), len(rr.pairs_within(1000.0))))
    ref = cj.combine(refs)
    r = mpc.screen(1000.0, samples_per_node=4, what="flown")
    print("planted pair:", r.pairs, "restated:", ref.pairs)
    assert r.n_pairs_total == 1 and r.pairs[:, :2].tolist() == [[a, b]] and ref.pairs[:, :2].tolist() == [[a, b]]
    assert 400.0 < r.pairs[0, 2] <= 500.001
    assert abs(r.pairs[0, 2] - ref.pairs[0, 2]) <= 1e-6 and abs(r.pairs[0, 3] - ref.pairs[0, 3]) <= 1e-6
    assert r.partner[a] == b and r.partner[b] == a
    close(r, ref)
    (wp,) = mpc._screen_windows("plan", samples_per_node=4)
    eph, status = R.ephemeris(wp["Y"], wp["units"], wp["span"], wp["M"], wp["T0"], wp["T1"], ns=wp["ns"])
    rp = mpc.screen(1000.0, samples_per_node=4, what="plan")
    assert (status == 0).all() and (rp.status == 0).all()
    close(rp, R.screen(eph, wp["T0"], wp["T1"]))
