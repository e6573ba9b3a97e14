"""The encounter window on the device (csrc/encounter_window.hip) against its numpy restatement (encounter_window_reference.py), in
both forms of the list and dealt over contexts, on the planted fast crossing against the closed form, on the planted slow pair, at
its edges and through ConstellationMPC.

Tolerances against the restatement, from the arithmetic.  The search's decisions are tests g <= 0; the restatement reports every
row's margin, the smallest |g| over every time it evaluated.  Two correct fp64 evaluations of g differ by the rounding of the node:
positions of 7e6 m through the Hermite's few operations differ by about 2e-7 m (test_conjunction_gpu.py), whitened by sigmas of 100 m
and more that is 2e-9, and |L^-1 d| of order 10 through a Cholesky factor adds 1e-14 cond(A): G0 is held to 1e-9 (1 + |G0|) and a row
whose margin exceeds 1e-9 is DECIDED -- both sides take the same cell at every level.  Its reaches then differ only by the fused
multiply-add in a + (l + 1) wd, a few ulp of an offset below H, and the window's ends by as much on a time of size |t|: 1e-13 (|t| + H)
is hundreds of ulp.  An undecided row may take the neighbouring cell at one level: two final cells, 2 H / 64^levels.  On these scenes
the restatement has no undecided row (measured on the CPU when written, H = 400: smallest margin 6.9 at levels = 1 for K = 3, 7.1
for K = 2, 6.3 for K = 30; at levels = 3 2.1e-4 for K = 2, 2.9e-5 for K = 3, 3.7e-4 for K = 30), which the test asserts."""
import functools

import numpy as np
import pytest

import collision_reference as C
import collision_window_reference as W
import encounter_window_reference as E
from test_collision_window_gpu import planted_fast, planted_slow, result_bits as window_bits

pytestmark = pytest.mark.gpu

H_SCENE = 400.0
DECIDED = 1e-9


def bits(r):
    return tuple(np.ascontiguousarray(x).tobytes() for x in (r.half, r.window, r.reach, r.g0, r.flags, r.status))


def scene_max_half(per_row):
    return np.where(np.arange(W.SCENE_N) % 2 == 0, H_SCENE, 250.0) if per_row else H_SCENE


@functools.lru_cache(maxsize=None)
def restated(K, levels, per_row):
    """the restatement of all 65 rows of window_scene(K) in the catalogue form: a row's result depends on the row alone, so the first
    n rows of it are the restatement of the list's first n rows.  Treat as read-only."""
    sc = W.window_scene(K)
    return E.encounter_window(sc["pairs"], sc["rows"], scene_max_half(per_row), 8.0, levels, sc["cat"])


def assert_close_to_restated(res, ref, t, H, levels, what):
    out, flags, status, margin = ref
    H = np.broadcast_to(np.asarray(H, dtype=np.float64), status.shape)
    assert np.array_equal(res.status, status) and (status == 0).all()
    got = np.column_stack([res.half, res.window, res.reach])
    err = np.abs(got - out[:, :E.EW_G0]).max(axis=1)
    gerr = np.abs(res.g0 - out[:, E.EW_G0])
    tight = 1e-13 * (np.abs(t) + H)
    decided = margin > DECIDED
    print(f"{what}: smallest margin {margin.min():.3e}, undecided rows {int((~decided).sum())} of {len(status)}, worst |error| / (1e-13 (|t| + H)) "
          f"{np.max(err / tight):.3f}, worst |dG0| / (1e-9 (1 + |G0|)) {np.max(gerr / (1e-9 * (1.0 + np.abs(out[:, E.EW_G0])))):.3f}")
    assert (gerr <= 1e-9 * (1.0 + np.abs(out[:, E.EW_G0]))).all()
    assert np.array_equal(res.flags[decided], flags[decided]) and (err[decided] <= tight[decided]).all()
    assert (err[~decided] <= 2.0 * H[~decided] / 64.0 ** levels).all()
    # a condition on the scenes, not a measurement: at most 5 % of the rows undecided -- and the restatement alone has none here
    assert (~decided).mean() <= 0.05
    assert decided.all(), f"{what}: the restatement has undecided rows, margins {margin[~decided]}"


@pytest.mark.parametrize("levels", [1, 3])
@pytest.mark.parametrize("per_row", [False, True], ids=["scalar", "per-row"])
@pytest.mark.parametrize("K", W.SCENE_KS)
@pytest.mark.parametrize("n", [1, 63, 65])
def test_encounter_window_against_the_restatement(n, K, per_row, levels):
    """the catalogue form of the first n rows of collision_window_reference.window_scene(K) -- km/s crossings and pairs below 1 m/s,
    one without any relative motion; ragged node counts; spans that cut the slow rows' live stretch where K is small --, max_half =
    400 s as a scalar and 400 / 250 s per row"""
    from mpconstellation_amd import encounter_window
    sc = W.window_scene(K)
    ref = tuple(x[:n] for x in restated(K, levels, per_row))
    Y, units, span, P, radius, _ = sc["rows"]
    H = scene_max_half(per_row)
    H = H[:n] if per_row else H
    res = encounter_window(sc["pairs"][:n], radius, Y, units, span, P, H, levels=levels, cat=sc["cat"])
    assert np.array_equal(res.pairs, sc["pairs"][:n])
    assert_close_to_restated(res, ref, sc["pairs"][:n, 3], H, levels, f"n {n} K {K} levels {levels} {'per-row' if per_row else 'scalar'}")
    assert np.array_equal(res.clear, (res.flags & 1) != 0) and np.array_equal(res.open, np.column_stack([(res.flags & 2) != 0, (res.flags & 4) != 0]))
    assert np.array_equal(res.half, np.maximum(res.reach[:, 0], res.reach[:, 1]))


def test_same_bits_in_both_forms_on_two_contexts_permuted_and_alone():
    from mpconstellation_amd import encounter_window
    sc = W.window_scene(30)
    Y, units, span, P, radius, _ = sc["rows"]
    H = scene_max_half(True)
    a = encounter_window(sc["pairs"], radius, Y, units, span, P, H, cat=sc["cat"])
    (uY, uunits, uspan, uP, uradius, uns), upairs = C.union_of(sc)
    b = encounter_window(upairs, uradius, uY, uunits, uspan, uP, H, ns=uns)
    c = encounter_window(sc["pairs"], radius, Y, units, span, P, H, cat=sc["cat"], devices=[0, 0])
    assert (a.status == 0).all() and bits(a) == bits(b) == bits(c)
    assert a.open.any() and not a.open.all()                               # (both kinds of row are in the list)
    perm = np.random.default_rng(3).permutation(W.SCENE_N)
    p = encounter_window(sc["pairs"][perm], radius, Y, units, span, P, H[perm], cat=sc["cat"])
    assert bits(p) == tuple(np.ascontiguousarray(x[perm]).tobytes() for x in (a.half, a.window, a.reach, a.g0, a.flags, a.status))
    for r in (0, 3, 18, 64):                                             # fast, the object that IS its satellite, slow, the last
        one = encounter_window(sc["pairs"][r:r + 1], radius, Y, units, span, P, H[r:r + 1], cat=sc["cat"])
        assert bits(one) == tuple(np.ascontiguousarray(x[r:r + 1]).tobytes() for x in (a.half, a.window, a.reach, a.g0, a.flags, a.status)), r


def test_planted_fast_crossing_against_the_closed_form():
    """test_collision_window_gpu.py's planted crossing (8.5 km/s, miss 300 m, combined isotropic sigma 282.84 m, R = 20 m) on the
    screen's own row, max_half 600 s, levels 3.  For a straight line and an isotropic constant covariance |L^-1 d| = sqrt(d0^2 +
    (speed h)^2) / sigma and |L^-1|_F = sqrt(3) / sigma, so g = 0 at h* = sqrt((nsigma sigma + sqrt(3) R)^2 - d0^2) / speed = 0.2673 s;
    the search returns the end of the final cell (600 / 64^3 = 0.0023 s) that holds it -- the restatement: 0.26779 s.  1e-3 relative
    allows for the screen's time offset and the orbit's curvature over a quarter of a second.  The window figure over .half then agrees
    with the short-encounter pc within the tolerance test_planted_fast_encounter_agrees_with_the_short_encounter_model derives: 10 x
    the two restatements' difference at this window plus the rounding bound, from the restatements alone."""
    from mpconstellation_amd import screen, collision_probability, collision_probability_window, encounter_window
    Y, units, spans, P, radius = planted_fast()
    scr = screen(Y=Y, units=units, span=spans, M=401, T0=0.0, T1=2000.0, threshold=1000.0)
    assert scr.pairs[:, :2].tolist() == [[0.0, 1.0]] and abs(scr.pairs[0, 3] - 1000.0) < 0.1
    col = collision_probability(scr, radius, Y, units, spans, P)
    ew = encounter_window(scr, radius, Y, units, spans, P, 600.0, levels=3)
    nsigma, R, cell = 8.0, radius.sum(), 600.0 / 64.0 ** 3
    hs = np.sqrt((nsigma * col.sigma[0, 0] + np.sqrt(3.0) * R) ** 2 - col.miss[0] ** 2) / col.speed[0]
    print(f"h* {hs:.6f} s, reaches {ew.reach[0]}, cell {cell:.6f} s, excess over h* in cells {(ew.reach[0] - hs) / cell}, g0 {ew.g0[0]:.6f}, flags {ew.flags[0]}")
    assert ew.status.tolist() == [0] and ew.flags.tolist() == [0] and ew.g0[0] < 0.0
    assert (ew.reach[0] >= hs * (1.0 - 1e-3)).all() and (ew.reach[0] <= hs * (1.0 + 1e-3) + cell).all()
    assert ew.half[0] == ew.reach[0].max() and np.array_equal(ew.window[0], [scr.pairs[0, 3] - ew.reach[0, 0], scr.pairs[0, 3] + ew.reach[0, 1]])
    side = (Y, units, spans, P, radius, None)
    ref_out, ref_flags, ref_st, _ = E.encounter_window(scr.pairs, side, 600.0, nsigma, 3)
    rounding = np.empty(1)
    ref_w, st_w = W.collision_probability_window(scr.pairs, side, ref_out[:, E.EW_HALF], 4, bounds=rounding)
    ref_c, st_c = C.collision_probability(scr.pairs, side)
    models = abs(ref_w[0, W.PW_P] - ref_c[0, 0]) / ref_c[0, 0]
    tol = 10.0 * models + rounding[0]
    win = collision_probability_window(scr, radius, Y, units, spans, P, ew.half, panels=4)
    print(f"half {ew.half[0]:.6f} s (restated {ref_out[0, E.EW_HALF]:.6f}), window p {win.p[0]:.12e}, short-encounter pc {col.pc[0]:.12e}, relative difference "
          f"{abs(win.p[0] - col.pc[0]) / col.pc[0]:.2e}; the restatements' {models:.2e}; tolerance {tol:.1e}")
    assert ref_st.tolist() == [0] and ref_flags.tolist() == [0] and st_w.tolist() == [0] and st_c.tolist() == [0]
    assert models <= 1.9e-7 and rounding[0] <= 1e-6 and tol <= 1e-4
    assert win.status.tolist() == [0] and abs(win.p[0] - col.pc[0]) <= tol * col.pc[0]


def test_planted_slow_pair_and_a_copy_of_itself_are_open():
    """test_collision_window_gpu.py's pair on one orbit (lag 150 m, 0.15 m/s) and an object against a copy of itself, t = 3000 s,
    max_half 600 s: both live all the way on both sides -- flags 6, HALF exactly 600.0, the window exactly [2400, 3600] --, and
    the window probability over .half has the bytes of the call with 600.0.  The restatement's g(t) of the lagging pair: -7.63."""
    from mpconstellation_amd import collision_probability_window, encounter_window
    Y, units, spans, P, radius = planted_slow()
    Y, units, spans, P, radius = (np.concatenate([x, x[:1]]) for x in (Y, units, spans, P, radius))       # object 2 = object 0
    pairs = np.array([[0.0, 1.0, 150.0, 3000.0], [0.0, 2.0, 0.0, 3000.0]])
    ref_out, ref_flags, ref_st, _ = E.encounter_window(pairs, (Y, units, spans, P, radius, None), 600.0, 8.0, 3)
    ew = encounter_window(pairs, radius, Y, units, spans, P, 600.0)
    print(f"g(t) {ew.g0}, restated {ref_out[:, E.EW_G0]}")
    assert ref_st.tolist() == [0, 0] and ref_flags.tolist() == [6, 6] and abs(ref_out[0, E.EW_G0] + 7.63) < 0.01
    assert ew.status.tolist() == [0, 0] and ew.flags.tolist() == [6, 6] and ew.open.all() and not ew.clear.any()
    assert ew.half.tolist() == [600.0, 600.0] and ew.reach.tolist() == [[600.0, 600.0]] * 2 and ew.window.tolist() == [[2400.0, 3600.0]] * 2
    assert (np.abs(ew.g0 - ref_out[:, E.EW_G0]) <= 1e-9 * (1.0 + np.abs(ref_out[:, E.EW_G0]))).all()
    a = collision_probability_window(pairs, radius, Y, units, spans, P, ew.half, panels=4)
    b = collision_probability_window(pairs, radius, Y, units, spans, P, 600.0, panels=4)
    assert a.status.tolist() == [0, 0] and window_bits(a) == window_bits(b)


def test_clear_row_gets_the_smallest_window():
    """A row whose own time is not live.  planted_slow's pair as it stands is live over its whole span (g(t) between -6.1 and -7.9:
    0.15 m/s moves it 450 m in 3000 s, about one sigma), so the pair here drifts at 3e-4 of the orbital speed (2.25 m/s, 1400 m below:
    live at t = 3000 s with g(t) = -5.2) and the row's time is the first of a few candidates at which the restatement puts g(t) > 1
    (5000 s: 3.3, measured on the CPU when written)."""
    from mpconstellation_amd import encounter_window
    Y, units, spans, P, radius = planted_slow(drift=3.0e-4)
    side = (Y, units, spans, P, radius, None)
    cand = np.array([[0.0, 1.0, 0.0, t] for t in (3000.0, 3500.0, 4000.0, 4500.0, 5000.0, 5500.0)])
    ref_out, ref_flags, ref_st, _ = E.encounter_window(cand, side, 600.0, 8.0, 3)
    assert ref_st.tolist() == [0] * 6 and ref_out[0, E.EW_G0] < 0.0 and ref_flags[0] & 1 == 0
    pick = np.flatnonzero(ref_out[:, E.EW_G0] > 1.0)
    assert len(pick), ref_out[:, E.EW_G0]
    row = cand[pick[0]:pick[0] + 1]
    print(f"t {row[0, 3]} s, restated g(t) {ref_out[pick[0], E.EW_G0]:.3f}")
    for levels in (1, 3, 4):
        ew = encounter_window(row, radius, Y, units, spans, P, 600.0, levels=levels)
        assert ew.status.tolist() == [0] and ew.flags.tolist() == [1] and ew.clear.tolist() == [True] and not ew.open.any()
        assert ew.reach.tolist() == [[600.0 / 64.0 ** levels] * 2] and ew.half[0] == 600.0 / 64.0 ** levels and ew.g0[0] > 1.0
        assert np.array_equal(ew.window[0], [row[0, 3] - ew.half[0], row[0, 3] + ew.half[0]])
    assert abs(ew.g0[0] - ref_out[pick[0], E.EW_G0]) <= 1e-9 * (1.0 + ref_out[pick[0], E.EW_G0])


def test_span_ends_close_the_window_without_an_open_flag():
    """the slow rows of the K = 3 scene (spans of 200 s and less, max_half 400 s): the live stretch runs into a span end, a scan time
    past it is not live, so no side is open, the window lies inside both spans and a reach is at most the distance to the span end
    plus one final cell"""
    from mpconstellation_amd import encounter_window
    sc = W.window_scene(3)
    slow = np.flatnonzero(np.arange(W.SCENE_N) % 4 >= 2)
    Y, units, span, P, radius, _ = sc["rows"]
    pairs = sc["pairs"][slow]
    ew = encounter_window(pairs, radius, Y, units, span, P, H_SCENE, levels=3, cat=sc["cat"])
    i, j, t = pairs[:, 0].astype(int), pairs[:, 1].astype(int), pairs[:, 3]
    lo, hi = np.maximum(span[i, 0], sc["cat"][2][j, 0]), np.minimum(span[i, 1], sc["cat"][2][j, 1])
    cell = H_SCENE / 64.0 ** 3
    assert (ew.status == 0).all() and not ew.open.any() and not ew.clear.any() and (ew.flags == 0).all()
    assert (ew.window[:, 0] >= lo).all() and (ew.window[:, 1] <= hi).all() and (ew.window[:, 0] < t).all() and (ew.window[:, 1] > t).all()
    assert (ew.reach[:, 0] <= t - lo + cell).all() and (ew.reach[:, 1] <= hi - t + cell).all()
    at_end = (ew.window[:, 0] == lo) | (ew.window[:, 1] == hi)
    print(f"{int(at_end.sum())} of {len(slow)} slow rows end at a span end")
    assert at_end.any()


def test_per_row_failures_leave_the_neighbours_alone():
    """a bad index, t outside a span, max_half 0, negative, NaN and inf, a radius that is not finite, an indefinite covariance at the
    row's own time: each failing row NaN in every column with flags 0 and the restatement's status, the good rows byte for byte what
    they are in a list of their own.  An indefinite covariance at a node that only scan times reach: flag 8, status 0."""
    from mpconstellation_amd import encounter_window
    sc = W.window_scene(30)
    (Y, units, span, P, radius, ns), pairs = C.union_of(sc)
    S = 5
    P, radius = P.copy(), radius.copy()
    rows = pairs[:22].copy()
    H = np.full(22, H_SCENE)
    P[S + 15] = -100.0 * P[S + 15]                                       # object 15: negative variances, larger than any satellite's
    radius[S + 17] = np.inf
    rows[1, 1] = len(Y)                                                  # no such object
    rows[3, 0] = -1.0
    rows[5, 3] = 1.0e6                                                   # outside both spans
    H[9], H[11], H[13], H[21] = 0.0, -5.0, np.nan, np.inf
    # row 19: object 19's covariance is indefinite two nodes away from the one nearest the row's time -- no time within half a node
    # interval (50 s) of t reads it, the scan to 400 s does
    o19, t19 = S + 19, rows[19, 3]
    hn = (span[o19, 1] - span[o19, 0]) / (ns[o19] - 1)
    kc = int(round((t19 - span[o19, 0]) / hn))
    kb = kc + 2 if kc + 2 < ns[o19] else kc - 2
    P[o19, kb] = -100.0 * P[o19, kb]
    good = [0, 2, 4, 6, 8, 10, 12, 14, 16, 18, 20]
    res = encounter_window(rows, radius, Y, units, span, P, H, ns=ns)
    ref_out, ref_flags, ref_status, margin = E.encounter_window(rows, (Y, units, span, P, radius, ns), H, 8.0, 3)
    B, N = C.ST_BADK, C.ST_NUMERIC
    assert ref_status.tolist() == [0, B, 0, B, 0, B, 0, 0, 0, B, 0, B, 0, B, 0, N, 0, N, 0, 0, 0, B]
    assert np.array_equal(res.status, ref_status)
    bad = res.status != 0
    for a in (res.half, res.window[:, 0], res.window[:, 1], res.reach[:, 0], res.reach[:, 1], res.g0):
        assert np.isnan(a[bad]).all() and np.isfinite(a[~bad]).all()
    assert (res.flags[bad] == 0).all()
    assert ref_flags[19] & 8 and res.flags[19] & 8 and res.status[19] == 0 and (res.flags[good] & 8 == 0).all()
    assert (margin[~bad] > DECIDED).all() and np.array_equal(res.flags, ref_flags)
    alone = encounter_window(rows[good], radius, Y, units, span, P, H[good], ns=ns)
    assert bits(alone) == tuple(np.ascontiguousarray(x[good]).tobytes() for x in (res.half, res.window, res.reach, res.g0, res.flags, res.status))


def test_c_abi_refuses_bad_sizes_nsigma_and_levels():
    from mpconstellation_amd import _ffi
    lib, ctx = _ffi.load(), _ffi.context(0)
    S, K, n = 2, 5, 3
    Y, units, span = np.zeros((S, 7, K)), np.ones((S, 2)), np.array([[0.0, 1.0]] * S)
    P, radius, pairs, half = np.zeros((S, K, 6, 6)), np.ones(S), np.zeros((n, 4)), np.ones(n)
    out, fl, pst = np.zeros((n, _ffi.NEW)), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    d, i = _ffi.dptr, _ffi.iptr
    row = lambda S, K: (S, K, None, d(Y), d(units), d(span), d(P), d(radius))
    none = (0, 0, None, None, None, None, None, None)

    def ew(n=n, rows=None, cols=none, mu=C.MU_EARTH, half=d(half), nsigma=8.0, levels=3, flags=i(fl)):
        return lib.mpcx_encounter_window(ctx, n, d(pairs), *(rows or row(S, K)), *cols, mu, half, nsigma, levels, d(out), flags, i(pst))
    for bad in (dict(n=0), dict(n=-1), dict(rows=row(0, K)), dict(rows=row(S, 1)), dict(mu=0.0), dict(mu=-1.0), dict(cols=row(0, K)),
                dict(cols=row(S, 1)), dict(cols=(S, K, None, d(Y), d(units), d(span), None, d(radius))), dict(half=None), dict(flags=None),
                dict(levels=0), dict(levels=_ffi.EW_MAX_LEVELS + 1), dict(nsigma=0.0), dict(nsigma=-1.0), dict(nsigma=np.nan),
                dict(nsigma=np.inf)):
        out[:] = 7.0
        assert ew(**bad) == -2, bad
        assert b"encounter_window" in lib.mpcx_last_error(ctx) and (out == 7.0).all()
    assert _ffi.EW_MAX_LEVELS == 4 and ew(levels=_ffi.EW_MAX_LEVELS) == 0 and ew(levels=1) == 0
    assert (pst == C.ST_NUMERIC).all() and np.isnan(out).all() and (fl == 0).all()       # (all zeros: no covariance to factor)


def test_constellation_mpc_chooses_the_window_with_auto():
    """test_collision_window_gpu.py's three-satellite plan with satellite 0 moved to pass 500 m from satellite 1: half_window='auto'
    returns the usual three results and the EncounterWindowResult, whose .half given as a number reproduces the window result byte
    for byte; the call with a number returns three results as before"""
    from mpconstellation_amd import Satellite, ConstellationMPC, EncounterWindowResult, conjunction as cj
    from mpconstellation_amd.constellation import constellation_states
    st = constellation_states(3)
    mpc = ConstellationMPC([Satellite(s[:3].copy(), s[3:6].copy(), float(s[6])) for s in st], base_res=30, tf_horizon=2, tf_interval=1, r_des=1.5)
    mpc.update()
    (w,) = mpc._screen_windows("plan", samples_per_node=4)
    X = mpc._plan[0]
    m = w["M"] // 3
    tb = w["T0"] + m * ((w["T1"] - w["T0"]) / (w["M"] - 1))
    side = (X, w["units"], w["span"], np.zeros((3, X.shape[2], 6, 6)), np.zeros(3), w["ns"])
    _, pa, va, _, _ = C.state_and_cov_at(side, 0, tb, C.MU_EARTH)
    _, pb, vb, _, _ = C.state_and_cov_at(side, 1, tb, C.MU_EARTH)
    e = np.cross(vb - va, [0.0, 0.0, 1.0]); e /= np.linalg.norm(e)
    X[0, 0:3, :] += ((pb - pa + 500.0 * e) / w["units"][0, 0])[:, None]
    P0 = np.diag([100.0 ** 2] * 3 + [0.1 ** 2] * 3)
    res = mpc.collision_probability_window(1000.0, P0, 5.0, "auto", panels=2, q=1e-8)
    assert len(res) == 4 and isinstance(res[3], EncounterWindowResult)
    scr, col, win, auto = res
    print("planted pair:", scr.pairs, "half", auto.half, "reach", auto.reach, "flags", auto.flags, "g0", auto.g0, "window p", win.p, "pc", col.pc)
    assert scr.pairs[:, :2].tolist() == [[0, 1]] and auto.status.tolist() == [0] and win.status.tolist() == [0] and 0.0 < win.p[0] < 1.0
    P = cj.covariance(X, w["units"], w["span"], mpc.consts, P0, U=mpc._plan[1], ns=w["ns"], q=1e-8)
    direct = cj.encounter_window(scr, 5.0, X, w["units"], w["span"], P, 0.5 * (w["T1"] - w["T0"]), ns=w["ns"])
    assert bits(direct) == bits(auto)
    numbered = mpc.collision_probability_window(1000.0, P0, 5.0, auto.half, panels=2, q=1e-8)
    assert len(numbered) == 3 and window_bits(numbered[2]) == window_bits(win) and numbered[1].pc.tobytes() == col.pc.tobytes()
    bounded = mpc.collision_probability_window(1000.0, P0, 5.0, "auto", panels=2, q=1e-8, max_half=20.0, nsigma=6.0)
    assert len(bounded) == 4 and (bounded[3].half <= 20.0).all() and bounded[3].status.tolist() == [0]
