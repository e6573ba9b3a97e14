"""Screening a constellation against a catalogue on the device (csrc/conjunction.hip) against its numpy restatement
(conjunction_cross_reference.py), and bit for bit against the all-pairs screen of the union.

Tolerances: those of test_conjunction_gpu.py (its `close`), which derives them -- partner identical (no ties, asserted),
|dmin - restated| <= 1e-6 m + 1e-12 dmin, |tca - restated| <= 1e-6 s (>= 1 m/s relative speed, asserted).
Shapes: a workgroup takes 64 rows below 512 rows and 256 from 512 on; the column tile is 16; the LDS chunk is 16 intervals in the
64-row kernel and 32 in the 256-row one -- one less, one more, not a multiple of each, and a launch whose column groups take more
than one tile each (catalogues beyond 2048 * 16 / waves objects)."""
import itertools

import numpy as np
import pytest

import conjunction_reference as R
import conjunction_cross_reference as X
from test_conjunction_gpu import bits, close

pytestmark = pytest.mark.gpu

SHAPES = list(itertools.product([1, 2, 63, 65, 255, 257], [1, 15, 17, 300], [2, 17, 130])) + [
    (65, 17, 33), (65, 17, 34),              # the LDS chunk of the 256-row kernel, here in the 64-row one
    (65, 17, 16), (65, 17, 18),              # the 64-row kernel's chunk of 16 intervals: one less, one more (17: above)
    (511, 17, 17), (512, 17, 18),            # the last 64-row launch, the first 256-row one (two full workgroups)
    (513, 17, 33), (513, 17, 34)]            # 256 rows: a third workgroup with one live lane; its chunk of 32 intervals


def against(c, **kw):
    from mpconstellation_amd import screen_against
    return screen_against(c["eph"], c["cat_eph"], c["T0"], c["T1"], **kw)


@pytest.mark.parametrize("S,D,M", SHAPES)
def test_against_the_restatement(S, D, M):
    from mpconstellation_amd import common_clock, screen_against
    c = X.case(S, D, M)
    X.assert_no_ties_and_moving(c)
    eph = common_clock(M=M, T0=c["T0"], T1=c["T1"], **c["sat"])
    cat = common_clock(c["cat"]["cat_Y"], c["cat"]["cat_units"], c["cat"]["cat_span"], M, c["T0"], c["T1"])
    assert np.abs(eph - c["eph"]).max() <= 1e-6 and np.abs(cat - c["cat_eph"]).max() <= 1e-6
    r = screen_against(eph, cat, c["T0"], c["T1"])
    close(r, c["ref"])
    assert r.status is None and r.cat_status is None and r.pairs.shape == (0, 4)
    close(against(c), c["ref"])                                      # the restated ephemerides in: the screen alone


@pytest.mark.parametrize("S,D,M", [(17, 40, 34), (65, 100, 130)])
def test_same_bits_as_the_union(S, D, M):
    """the pair (i, j) is the pair (i, S + j) of the union [constellation; catalogue]: the same kernel text with and without SELF,
    the same operands"""
    from mpconstellation_amd import screen
    c = X.case(S, D, M)
    X.assert_no_ties_and_moving(c)
    u = screen(np.concatenate([c["eph"], c["cat_eph"]]), c["T0"], c["T1"], threshold=1e9, max_pairs=20000)
    assert u.n_pairs_total == (S + D) * (S + D - 1) // 2 == len(u.pairs)
    rows = u.pairs[(u.pairs[:, 0] < S) & (u.pairs[:, 1] >= S)].copy()
    rows[:, 1] -= S
    r = against(c, threshold=1e9)
    assert r.n_pairs_total == S * D and r.pairs.tobytes() == rows.tobytes()
    dmin, partner, tca = np.empty(S), np.empty(S, dtype=np.int32), np.empty(S)
    for i in range(S):
        mine = rows[rows[:, 0] == i]
        k = np.argmin(mine[:, 2])                                    # the first minimum: the smaller catalogue index (rows are sorted)
        dmin[i], partner[i], tca[i] = mine[k, 2], mine[k, 1], mine[k, 3]
    assert r.dmin.tobytes() == dmin.tobytes() and r.partner.tobytes() == partner.tobytes() and r.tca.tobytes() == tca.tobytes()


def test_fused_and_several_devices_hold_the_same_bits():
    from mpconstellation_amd import common_clock, screen_against
    c = X.case(257, 300, 130)
    thr = np.sort(c["ref"].pairs[:, 2])[20]
    eph = common_clock(M=130, T0=c["T0"], T1=c["T1"], **c["sat"])
    cat = common_clock(c["cat"]["cat_Y"], c["cat"]["cat_units"], c["cat"]["cat_span"], 130, c["T0"], c["T1"])
    two_step = screen_against(eph, cat, c["T0"], c["T1"], threshold=thr)
    traj = dict(M=130, T0=c["T0"], T1=c["T1"], threshold=thr, **c["sat"], **c["cat"])
    fused = screen_against(**traj)
    assert two_step.n_pairs_total >= 20 and bits(fused) == bits(two_step)
    assert (fused.status == 0).all() and fused.status.shape == (257,) and (fused.cat_status == 0).all() and fused.cat_status.shape == (300,)
    assert bits(screen_against(eph, cat, c["T0"], c["T1"], threshold=thr, devices=[0, 0])) == bits(two_step)
    assert bits(screen_against(devices=[0, 0, 0], **traj)) == bits(two_step)


@pytest.mark.parametrize("S", [511, 513])
def test_column_groups_that_take_several_tiles(S):
    """4113 objects are 258 column tiles: more than the 256 column groups of the 64-row launch of 511 rows, and than the 171 of
    the 256-row launch of 513.  Each half of the catalogue alone is one tile per group, the path the restatement comparison
    covers; the minimum under the total order over the two halves must be the whole catalogue's, bit for bit."""
    from mpconstellation_amd import screen_against
    D, M, half = 4113, 18, 2056
    orb = R.random_orbits(S + D, seed=S)
    T0, T1 = 0.0, 2 * np.pi / R.orbit_rate(orb).max()
    p, v = R.kepler_state({k: x[:, None] for k, x in orb.items()}, np.linspace(T0, T1, M)[None, :])      # (S + D, M, 3)
    eph = np.ascontiguousarray(np.concatenate([p, v], axis=2).transpose(0, 2, 1))
    whole = screen_against(eph[:S], eph[S:], T0, T1, threshold=1.0e5, max_pairs=1 << 18)
    a = screen_against(eph[:S], eph[S:S + half], T0, T1, threshold=1.0e5, max_pairs=1 << 18)
    b = screen_against(eph[:S], eph[S + half:], T0, T1, threshold=1.0e5, max_pairs=1 << 18)
    assert (a.partner >= 0).all() and (b.partner >= 0).all() and 100 <= whole.n_pairs_total < 1 << 18
    first = a.dmin <= b.dmin                                         # (equal distances: the smaller catalogue index, the first half's)
    assert np.array_equal(whole.dmin, np.where(first, a.dmin, b.dmin)) and np.array_equal(whole.tca, np.where(first, a.tca, b.tca))
    assert np.array_equal(whole.partner, np.where(first, a.partner, b.partner + half))
    pb = b.pairs.copy(); pb[:, 1] += half
    from mpconstellation_amd.conjunction import sort_pairs
    assert whole.n_pairs_total == a.n_pairs_total + b.n_pairs_total
    assert whole.pairs.tobytes() == sort_pairs(np.concatenate([a.pairs, pb])).tobytes()


def test_pairs_list():
    c = X.case(65, 300, 130)
    ref = c["ref"]
    d = np.sort(ref.pairs[:, 2])
    thr = 0.5 * (d[9] + d[10])                                      # the ten closest of the 19 500 pairs
    assert d[10] - d[9] > 1e-3
    want = ref.pairs_within(thr)
    r = against(c, threshold=thr)
    assert r.n_pairs_total == 10 and np.array_equal(r.pairs[:, :2], want[:, :2])
    assert (np.abs(r.pairs[:, 2] - want[:, 2]) <= 1e-6 + 1e-12 * want[:, 2]).all() and (np.abs(r.pairs[:, 3] - want[:, 3]) <= 1e-6).all()
    cut = against(c, threshold=thr, max_pairs=4)
    assert cut.n_pairs_total == 10 and cut.pairs.shape == (4, 4)
    full = {tuple(row) for row in r.pairs.tolist()}
    assert all(tuple(row) in full for row in cut.pairs.tolist())
    assert np.array_equal(cut.dmin, r.dmin) and np.array_equal(cut.partner, r.partner) and np.array_equal(cut.tca, r.tca)
    none = against(c)
    assert none.n_pairs_total == 0 and none.pairs.shape == (0, 4)


def test_spans_that_miss_the_grid_on_both_sides():
    from mpconstellation_amd import screen_against
    S, D, M, n = 17, 12, 40, 30
    orb = R.random_orbits(S + D, seed=5)
    T0, T1 = 0.0, 3000.0
    span = np.tile([T0 - 1.0, T1 + 1.0], (S + D, 1))
    span[3] = (T1 + 100.0, T1 + 2000.0)                              # a satellite that is never on the grid
    span[9] = (T0 - 500.0, 1500.0)                                   # a satellite that is there for the first half
    span[S + 4] = (T1 + 100.0, T1 + 2000.0)                          # an object that is never on the grid
    span[S + 7] = (1500.0, 1560.0)                                   # an object that sees one instant only
    span[S + 2] = (1000.0, 2100.0)
    Y, units, span = R.trajectories(orb, n, span)
    eph_ref, _ = R.ephemeris(Y, units, span, M, T0, T1)
    assert np.isnan(eph_ref[3]).all() and np.isnan(eph_ref[S + 4]).all() and (~np.isnan(eph_ref[S + 7, 0])).sum() == 1
    ref = X.screen_against(eph_ref[:S], eph_ref[S:], T0, T1)
    r = screen_against(eph_ref[:S], eph_ref[S:], T0, T1, threshold=1e9)
    close(r, ref)
    assert r.partner[3] == -1 and np.isposinf(r.dmin[3]) and np.isnan(r.tca[3])
    assert not (r.partner == 4).any() and not (r.partner == 7).any() and (np.delete(r.partner, 3) >= 0).all()
    assert np.array_equal(r.pairs[:, :2], ref.pairs[:, :2]) and r.n_pairs_total == (S - 1) * (D - 2)
    assert not (r.pairs[:, 0] == 3).any() and not np.isin(r.pairs[:, 1], [4, 7]).any()
    f = screen_against(Y=Y[:S], units=units[:S], span=span[:S], cat_Y=Y[S:], cat_units=units[S:], cat_span=span[S:], M=M, T0=T0, T1=T1)
    close(f, ref)
    assert (f.status == 0).all() and (f.cat_status == 0).all()


def test_ragged_counts_ignore_what_lies_past_them():
    from mpconstellation_amd import screen_against
    c = X.case(17, 15, 17)
    n, k, kc = 40, 23, 31
    orb = c["orb"]
    pick = lambda a, b: {key: v[a:b] for key, v in orb.items()}
    Yk, units, span = R.trajectories(pick(0, 17), k, c["sat"]["span"])
    Ck, cunits, cspan = R.trajectories(pick(17, 32), kc, c["cat"]["cat_span"])
    Yg = np.full((17, 7, n), 1e300); Yg[:, :, :k] = Yk; Yg[3, :, k:] = np.nan
    Cg = np.full((15, 7, n), 1e300); Cg[:, :, :kc] = Ck; Cg[5, :, kc:] = np.nan
    grid = dict(M=17, T0=c["T0"], T1=c["T1"], threshold=1e9)
    ra = screen_against(Y=Yk, units=units, span=span, cat_Y=Ck, cat_units=cunits, cat_span=cspan, **grid)
    rb = screen_against(Y=Yg, units=units, span=span, ns=np.full(17, k), cat_Y=Cg, cat_units=cunits, cat_span=cspan, cat_ns=np.full(15, kc), **grid)
    assert bits(ra) == bits(rb) and ra.n_pairs_total == 17 * 15 and not np.isnan(ra.dmin).any()
    assert (rb.status == 0).all() and (rb.cat_status == 0).all()


def test_bad_counts_are_reported_on_their_side():
    from mpconstellation_amd import screen_against
    c = X.case(2, 15, 17)
    span = c["sat"]["span"].copy(); span[1] = (5.0, 5.0)
    cat_ns = np.full(15, 40); cat_ns[[2, 6]] = (1, 41)
    r = screen_against(Y=c["sat"]["Y"], units=c["sat"]["units"], span=span, cat_ns=cat_ns, M=17, T0=c["T0"], T1=c["T1"], threshold=1e9, **c["cat"])
    assert r.status.tolist() == [0, 9] and r.cat_status.tolist() == [9 if j in (2, 6) else 0 for j in range(15)]
    assert r.partner[1] == -1 and r.partner[0] >= 0 and not np.isin(r.pairs[:, 1], [2, 6]).any() and r.n_pairs_total == 13


def test_an_object_on_a_satellites_trajectory_gives_zero():
    from mpconstellation_amd import screen_against
    c = X.case(2, 15, 17)
    cat = {k: v.copy() for k, v in c["cat"].items()}
    for k in cat:
        cat[k][3] = c["sat"][k[4:]][0]
    r = screen_against(M=17, T0=c["T0"], T1=c["T1"], **c["sat"], **cat)
    assert r.dmin[0] == 0.0 and r.partner[0] == 3 and r.dmin[1] > 0.0


def test_c_abi_refuses_bad_arguments():
    from mpconstellation_amd import _ffi
    lib, ctx = _ffi.load(), _ffi.context(0)
    eph = np.zeros((2, 6, 4)); cat = np.zeros((3, 6, 4)); d = np.zeros(2); p = np.zeros(2, dtype=np.int32); t = np.zeros(2)
    pairs = np.zeros((4, 4)); n = np.zeros(1, dtype=np.int64)
    out = (_ffi.dptr(d), _ffi.iptr(p), _ffi.dptr(t), _ffi.dptr(pairs), n.ctypes.data_as(_ffi._lp))
    good = dict(S=2, D=3, M=4, T0=0.0, T1=1.0, row0=0, nrows=2, thr=1.0, max_pairs=4)

    def call(a, tail=out):
        return lib.mpcx_conjunction_cross_screen(ctx, a["S"], a["D"], a["M"], _ffi.dptr(eph), _ffi.dptr(cat), a["T0"], a["T1"], a["row0"], a["nrows"],
                                                 a["thr"], a["max_pairs"], *tail)
    assert call(good) == 0 and n[0] == 6                             # (all zeros: every one of the 2 x 3 pairs at distance 0)
    for bad in (dict(D=0), dict(S=0), dict(M=1), dict(T1=0.0), dict(T1=-1.0), dict(max_pairs=-1), dict(row0=1), dict(nrows=3), dict(nrows=0)):
        assert call({**good, **bad}) == -2, bad
        assert b"conjunction_cross_screen" in lib.mpcx_last_error(ctx)
    assert call(good, out[:4] + (None,)) == -2                       # a threshold without n_pairs
    assert call({**good, "thr": 0.0, "max_pairs": 0}, out[:3] + (None, None)) == 0
    Y = np.zeros((2, 7, 5)); u = np.ones((2, 2)); sp = np.array([[0.0, 1.0]] * 2); st = np.zeros(2, dtype=np.int32)
    cY = np.zeros((3, 7, 6)); cu = np.ones((3, 2)); csp = np.array([[0.0, 1.0]] * 3); cst = np.zeros(3, dtype=np.int32)
    for S, D, M, T1 in ((0, 3, 4, 1.0), (2, 0, 4, 1.0), (2, 3, 1, 1.0), (2, 3, 4, 0.0)):
        rc = lib.mpcx_conjunction_cross_screen_traj(ctx, S, 5, None, _ffi.dptr(Y), _ffi.dptr(u), _ffi.dptr(sp), D, 6, None, _ffi.dptr(cY), _ffi.dptr(cu),
                                                    _ffi.dptr(csp), M, 0.0, T1, 0, 2, 0.0, 0, *out, _ffi.iptr(st), _ffi.iptr(cst))
        assert rc == -2, (S, D, M, T1)
    w = lib.mpcx_conjunction_cross_workspace_bytes
    assert w(2, 0, 4) == 0 and w(0, 3, 4) == 0 and w(2, 3, 1) == 0 and w(2, 3, 4) > 0


def test_constellation_against_a_planted_object():
    """64 satellites flown for two segments; the catalogue is three of their second-segment trajectories moved away: two by 50 km,
    the third so that it passes about 500 m from satellite 5, across the relative motion, at a node of the second segment.
    screen_against(cat, 1000) lists exactly that pair, as the restatement does on the same windows; in the first window no
    object is inside its span.  Every row is held to the restatement within the file's tolerances, except the tca of satellite 20:
    its nearest object is its own trajectory moved by 50 km, so the relative velocity is zero, the distance is the same at every
    instant, and the bound on tca, which is the distance bound divided by a relative speed of at least 1 m/s, says nothing there."""
    from mpconstellation_amd import Satellite, ConstellationMPC, conjunction as cj
    from mpconstellation_amd.constellation import constellation_states
    st = constellation_states(64)
    mpc = ConstellationMPC([Satellite(s[:3].copy(), s[3:6].copy(), float(s[6])) for s in st], base_res=30, tf_horizon=2, tf_interval=1,
                           r_des=1.5, sim_base_res=100)
    mpc.run_segments(tf=2, num_segments=2)
    windows = mpc._screen_windows("flown", samples_per_node=4)
    src, a, k = [5, 20, 40], 5, 37
    y = mpc._seg_y[1]
    cat_Y, cat_units, cat_span = y[src].copy(), windows[1]["units"][src].copy(), windows[1]["span"][src].copy()
    L = cat_units[:, 0]; V = L / cat_units[:, 1]
    La = windows[1]["units"][a, 0]; Va = La / windows[1]["units"][a, 1]
    w = cat_Y[2, 3:6, k] * V[2] - y[a, 3:6, k] * Va                  # relative velocity at the planted instant (m/s)
    e = np.cross(w, [0.0, 0.0, 1.0]); e /= np.linalg.norm(e)         # the miss vector: across the relative motion
    assert np.linalg.norm(w) >= 1.0
    cat_Y[0, 0, :] += 5.0e4 / L[0]
    cat_Y[1, 2, :] += 5.0e4 / L[1]
    cat_Y[2, 0:3, :] += ((y[a, 0:3, k] * La - cat_Y[2, 0:3, k] * L[2] + 500.0 * e) / L[2])[:, None]
    cat = (cat_Y, cat_units, cat_span)

    def restated(wdw):
        eph, _ = R.ephemeris(wdw["Y"], wdw["units"], wdw["span"], wdw["M"], wdw["T0"], wdw["T1"], ns=wdw["ns"])
        ceph, _ = R.ephemeris(cat_Y, cat_units, cat_span, wdw["M"], wdw["T0"], wdw["T1"])
        rr = X.screen_against(eph, ceph, wdw["T0"], wdw["T1"])
        return cj.ConjunctionResult(rr.dmin, rr.partner, rr.tca, rr.pairs_within(1000.0), len(rr.pairs_within(1000.0)))
    refs = [restated(wdw) for wdw in windows]
    assert (refs[0].partner == -1).all() and (refs[1].partner >= 0).all()
    ref = cj.combine(refs)
    r = mpc.screen_against(cat, 1000.0, samples_per_node=4, what="flown")
    print("planted pair:", r.pairs, "restated:", ref.pairs)
    assert r.n_pairs_total == 1 and r.pairs[:, :2].tolist() == [[a, 2]] and ref.pairs[:, :2].tolist() == [[a, 2]]
    assert 400.0 < r.pairs[0, 2] <= 500.001
    assert abs(r.pairs[0, 2] - ref.pairs[0, 2]) <= 1e-6 and abs(r.pairs[0, 3] - ref.pairs[0, 3]) <= 1e-6
    assert r.partner[a] == 2
    # satellite 20's nearest object is its own trajectory moved by 50 km: zero relative velocity, a constant distance whose
    # smallest instant the rounding decides -- the bound on tca assumes >= 1 m/s and does not apply to that row; every other
    # row's partner moves past it
    assert ref.partner[20] == 1 and ref.partner[a] == 2              # (the other moved trajectory, satellite 5's, is not 5's nearest)
    assert r.partner[20] == 1 and abs(r.dmin[20] - ref.dmin[20]) <= 1e-6 + 1e-12 * ref.dmin[20] and abs(r.dmin[20] - 5.0e4) < 1e-3
    moving = np.arange(64) != 20
    close(cj.ConjunctionResult(r.dmin[moving], r.partner[moving], r.tca[moving], r.pairs, 1),
          cj.ConjunctionResult(ref.dmin[moving], ref.partner[moving], ref.tca[moving], ref.pairs, 1))
    (wp,) = mpc._screen_windows("plan", samples_per_node=4)
    rp = mpc.screen_against(cat, 1000.0, samples_per_node=4, what="plan")
    assert (rp.status == 0).all() and (rp.cat_status == 0).all()
    close(rp, restated(wp))


def test_catalogue_trajectories():
    from mpconstellation_amd import SatelliteScale, catalogue_trajectories, propagate_batch, _ffi
    D, n, T0, T1 = 5, 30, 100.0, 3100.0
    orb = R.random_orbits(D, seed=11)
    p, v = R.kepler_state(orb, np.zeros(D))
    Y, units, span = catalogue_trajectories(p, v, T0, T1, n)
    radius = np.linalg.norm(p, axis=1)
    assert np.array_equal(units[:, 0], radius) and np.allclose(units[:, 1], 2 * np.pi * np.sqrt(radius ** 3 / R.MU_EARTH), rtol=1e-15, atol=0.0)
    assert np.array_equal(span, np.tile([T0, T1], (D, 1))) and Y.shape == (D, 7, n)
    V = units[:, 0] / units[:, 1]
    assert np.abs(Y[:, 0:3, 0] * units[:, 0:1] - p).max() <= 1e-12 * radius.min() and np.abs(Y[:, 3:6, 0] * V[:, None] - v).max() <= 1e-12 * 7.5e3
    # the same call made here: the objects' own scales, zero thrust, no drag
    scales = [SatelliteScale(x=np.concatenate([p[s], v[s], [1.0]])) for s in range(D)]
    y0 = np.stack([sc.normalize_state(np.concatenate([p[s], v[s], [1.0]])) for s, sc in enumerate(scales)])
    consts = np.stack([sc.get_normalized_constants().as_vector() for sc in scales])
    tf = np.array([(T1 - T0) / sc.units["time"] for sc in scales])
    direct, status, _ = propagate_batch(y0, tf, consts, (_ffi.CTRL_ZERO, None, 0, 1.0), n, include_drag=False, include_J2=True)
    assert (status == 0).all() and Y.tobytes() == direct.tobytes()
