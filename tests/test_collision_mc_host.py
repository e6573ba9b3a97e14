"""The Monte Carlo collision probability without a device: the numpy restatement (collision_mc_reference) of the generator, the draws
and the scan against known answers and closed forms, and what conjunction.collision_probability_mc and ConstellationMPC hand on, with
the recorder of test_wrapper_calls_host.py in place of the library."""
import numpy as np
import pytest

import collision_mc_reference as M
import collision_reference as C
import covariance_thrust_reference as T
from mpconstellation_amd import _ffi, conjunction as cj
from test_wrapper_calls_host import I32, Out, check_call, f64, i32, rec      # noqa: F401 (rec: the fixture)


def words(c):
    return " ".join(f"{int(x):08x}" for x in c)


def test_generator_known_answers():
    """Philox4x32-10: the three known answers of the published test vectors (zero, all ones, the digits of pi)"""
    F = 0xFFFFFFFF
    assert words(M.philox(0, 0, 0, 0, 0, 0)) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert words(M.philox(F, F, F, F, F, F)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert words(M.philox(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)) == "d16cfe09 94fdcceb 5001e420 24126ea1"
    many = M.philox(np.arange(5), 0, 0, 0, 0, 0)                       # arrays of counters: element 0 is the scalar's
    assert [int(w[0]) for w in many] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8] and len(set(int(x) for x in many[0])) == 5


def test_uniforms_stay_strictly_inside_the_unit_interval():
    """all-zero words give 2^-54, all-one words 1 - 2^-53 (the exact value 1 - 2^-54 is a tie, rounded down); both normals are finite
    at both ends; the mapping is monotone across the rounding region above 2^52"""
    F = 0xFFFFFFFF
    lo, hi = float(M.uniform(0, 0)), float(M.uniform(F, F))
    assert lo == 2.0 ** -54 and hi == 1.0 - 2.0 ** -53 and 0.0 < lo < hi < 1.0
    a = np.array([0, 1 << 5, 0x7FFFFFFF, 0x80000000, F, F], dtype=np.uint64)
    b = np.array([1 << 6, 0, F, 0, F - 64, F], dtype=np.uint64)
    u = M.uniform(a, b)
    assert (np.diff(u) >= 0.0).all() and (u > 0.0).all() and (u < 1.0).all()
    for x in (lo, hi):
        r = np.sqrt(-2.0 * np.log(x))
        assert np.isfinite(r) and r >= 0.0


def test_factor_rule():
    """the planted fast scene's P0 has no velocity uncertainty: three regular pivots, three zero pivots.  A correlated rank-3 matrix is
    reproduced by L L^T; an indefinite matrix, a negative variance, a NaN and a zero pivot under a non-zero column are refused."""
    P0 = np.diag([200.0 ** 2] * 3 + [0.0] * 3)
    ok, L = M.factor(P0)
    assert ok and np.array_equal(L, np.diag([200.0] * 3 + [0.0] * 3))
    rng = np.random.default_rng(3)
    G = rng.normal(size=(6, 3)) * np.array([100.0] * 3 + [0.1] * 3)[:, None]
    G[1] = 0.0                                                         # a zero row: a zero pivot in the middle
    P = G @ G.T
    ok, L = M.factor(P)
    assert ok and np.abs(L @ L.T - P).max() <= 1e-9 * np.abs(P).max() and np.array_equal(L, np.tril(L)) and (L[:, 1] == 0.0).all()
    ok, L = M.factor(C.P0_TEST)
    assert ok and np.abs(L @ L.T - C.P0_TEST).max() <= 1e-13 * np.abs(C.P0_TEST).max()
    assert np.abs(L - np.linalg.cholesky(C.P0_TEST)).max() <= 1e-12 * np.abs(L).max()
    bad = [np.diag([1.0, -1.0, 1.0, 1.0, 1.0, 1.0]), np.diag([1.0, np.nan, 1.0, 1.0, 1.0, 1.0]), np.diag([1.0, np.inf, 1.0, 1.0, 1.0, 1.0])]
    ind = np.eye(6); ind[0, 1] = ind[1, 0] = 2.0                       # indefinite
    col = np.diag([1.0, 0.0, 1.0, 1.0, 1.0, 1.0]); col[1, 3] = col[3, 1] = 0.5      # a zero variance that is correlated
    for P in bad + [ind, col]:
        assert not M.factor(P)[0]
    lower = C.P0_TEST.copy(); lower[np.tril_indices(6, -1)] = np.nan   # only the upper triangle is read
    assert M.factor(lower)[0]


def covariance_tolerance(S, N, k=5.0):
    """k standard errors of the entries of a sample covariance about a KNOWN mean of N Gaussian samples with covariance S:
    Var(mean of x_i x_j) = (S_ii S_jj + S_ij^2) / N"""
    d = np.diag(S)
    return k * np.sqrt((np.outer(d, d) + S * S) / N)


def test_draw_moments():
    """10^5 Gates draws at a node reproduce covariance_thrust_reference.sigma, and 10^5 state draws reproduce P0, entry by entry
    within 5 standard errors of a sample covariance about the known mean (covariance_tolerance); a node at or below u_off and
    execution=None add nothing; the frame is orthonormal and right-handed; different objects, sides and seeds draw differently."""
    N = 100000
    s = np.arange(N)
    ex = np.array([1e-4, 0.02, 1e-4, 0.01745, 1e-3])
    U = np.array([[0.013, 0.0, 3e-4], [-0.02, 0.0, -4e-4], [0.007, 0.0, 0.0]])     # node 1 is off, node 2 is below u_off
    out, bound = M.draw_thrust(U, 3, ex, s, 5, 0, 77)
    for k in (0,):
        e = out[:, :, k] - U[None, :, k]
        S = T.sigma(U[:, k], ex)
        got = e.T @ e / N
        tol = covariance_tolerance(S, N)
        print(f"Gates draw: worst |sample - Sigma| / tolerance {np.max(np.abs(got - S) / tol):.3f}")
        assert (np.abs(got - S) <= tol).all() and np.abs(e.mean(0)).max() <= 5.0 * np.sqrt(np.diag(S).max() / N)
        assert np.abs(M.gates_sigma(U[:, k], ex) - S).max() <= 1e-15 * np.abs(S).max()
    assert np.array_equal(out[:, :, 1], np.zeros((N, 3))) and np.array_equal(out[:, :, 2], np.broadcast_to(U[:, 2], (N, 3)))
    assert (bound[:, :, 1:] == 0.0).all() and bound[:, :, 0].max() < 1e-15
    plain, _ = M.draw_thrust(U, 3, None, s[:4], 5, 0, 77)
    assert np.array_equal(plain, np.broadcast_to(U, (4, 3, 3)))
    cut, _ = M.draw_thrust(U, 1, ex, s[:4], 5, 0, 77)
    assert np.array_equal(cut[:, :, 0], out[:4, :, 0]) and (cut[:, :, 1:] == 0.0).all()       # past the node count: zero
    for u in (U[:, 0], np.array([0.0, 0.0, 1.0]), np.array([1.0, 1.0, 1.0]), np.array([-1.0, 1.0, 0.5])):
        un, h, e1, e2 = M.gates_frame(u)
        Q = np.stack([h, e1, e2])
        assert np.abs(Q @ Q.T - np.eye(3)).max() <= 4e-16 and np.linalg.det(Q) > 0.0
    assert np.array_equal(M.gates_frame(np.array([1.0, 1.0, 1.0]))[2], M.gates_frame(np.array([2.0, 2.0, 2.0]))[2])
    assert M.gates_frame(np.array([1.0, 1.0, 1.0]))[2][0] > 0.8      # the FIRST of equal axes
    # the state
    units = np.array([7.0e6, 5800.0])
    y1 = np.array([1.0, 0.0, 0.0, 0.0, 6.28, 0.0, 1.0])
    ok, y0, b = M.draw_initial(y1, units, C.P0_TEST, 1e-4, s, 2, 0, 77)
    D = np.array([units[0]] * 3 + [units[0] / units[1]] * 3)
    x = (y0[:, :6] - y1[None, :6]) * D
    got = x.T @ x / N
    tol = covariance_tolerance(C.P0_TEST, N) + 1e-6 * np.abs(C.P0_TEST)             # (the subtraction from y1 rounds at 1e-16 of 7e6 m)
    print(f"state draw: worst |sample - P0| / tolerance {np.max(np.abs(got - C.P0_TEST) / tol):.3f}")
    assert ok and (np.abs(got - C.P0_TEST) <= tol).all()
    m = y0[:, 6] - 1.0
    assert abs(m.var() - 1e-4) <= 5.0 * 1e-4 * np.sqrt(2.0 / N) and abs(m.mean()) <= 5.0 * 1e-2 / np.sqrt(N)
    assert abs(np.corrcoef(m, x[:, 0])[0, 1]) <= 5.0 / np.sqrt(N)
    assert b.max() <= 1e-12
    for other in (dict(obj=3), dict(side=1), dict(seed=78), dict(seed=77 + (1 << 32))):
        kw = dict(obj=2, side=0, seed=77); kw.update(other)
        _, y2, _ = M.draw_initial(y1, units, C.P0_TEST, 1e-4, s[:8], kw["obj"], kw["side"], kw["seed"])
        assert not np.array_equal(y2, y0[:8]), other
    _, y2, _ = M.draw_initial(y1, units, C.P0_TEST, 1e-4, s[5:8], 2, 0, 77)        # a sample's draws do not depend on its neighbours
    assert np.array_equal(y2, y0[5:8])


def test_scan_on_straight_paths_gives_the_closed_form_hit():
    """test_slow_encounter_against_monte_carlo's paths (slow_case: rho(t) = rho_0 + nu t, drawn as there from seed 7, the first 3000):
    a line enters the sphere at most once, and the sample hits iff its closest point over [0, T] is within R.  The scan (64
    intervals; 1 and 7 too: the cubic Hermite of a line is the line) gives that hit, at most one entry, the closed form's distance
    and time, for every sample not within 1e-6 m of R at its closest point."""
    from test_collision_window_host import slow_case
    R, d0, w, A0, B0, D0, Tw = slow_case()
    rng = np.random.default_rng(7)
    cov = np.block([[A0, B0.T], [B0, D0]])
    x = rng.multivariate_normal(np.concatenate([d0, w]), cov, size=400000, method="cholesky")[:3000]
    r0, nu = x[:, 0:3], x[:, 3:6]
    ts = np.clip(-(r0 * nu).sum(1) / (nu * nu).sum(1), 0.0, Tw)
    dist = np.linalg.norm(r0 + nu * ts[:, None], axis=1)
    clear = np.abs(dist - R) > 1e-6
    assert clear.sum() >= 2990 and 50 <= (dist <= R).sum() <= 300
    for scan in (64, 7, 1):
        t = M.scan_instants(0.0, Tw, scan)
        assert t[0] == 0.0 and t[-1] == Tw and len(t) == scan + 1
        for s in np.flatnonzero(clear)[:3000 if scan == 64 else 300]:
            (dmin, tmin, ins, ent), _, _ = M.scan_relative(t, r0[s][None, :] + nu[s][None, :] * t[:, None], np.broadcast_to(nu[s], (scan + 1, 3)), R)
            assert (ins == 1 or ent >= 1) == bool(dist[s] <= R), (scan, s)
            assert ent <= 1 and ins == int(np.linalg.norm(r0[s]) <= R) and not (ins and ent)
            assert abs(dmin - dist[s]) <= 1e-9 * (1.0 + dist[s]) and abs(tmin - ts[s]) <= 1e-6 * Tw, (scan, s, dmin, dist[s])


def test_scan_counts_two_entries_and_one_hit_on_a_path_that_crosses_twice():
    """rho(t) = (60 cos wt, 20, 0) m over one period, R = 50 m: outside at the start (63 m), inside around a quarter and three quarters
    of the period (20 m), outside in between -> inside_start 0, 2 entries, 1 hit; over the last three quarters, started inside:
    inside_start 1, 1 entry; with ONE scan interval over the whole period the two entries are one (the resolution the header says scan must buy)"""
    Tp, R = 6000.0, 50.0
    om = 2.0 * np.pi / Tp

    def path(t):
        return (np.stack([60.0 * np.cos(om * t), np.full_like(t, 20.0), np.zeros_like(t)], axis=1),
                np.stack([-60.0 * om * np.sin(om * t), np.zeros_like(t), np.zeros_like(t)], axis=1))
    t = M.scan_instants(0.0, Tp, 64)
    (dmin, tmin, ins, ent), q_ends, qm = M.scan_relative(t, *path(t), R)
    assert (ins, ent) == (0, 2) and abs(dmin - 20.0) <= 1e-6 and abs(tmin - Tp / 4.0) <= 1e-6 * Tp       # the earliest of the two minima
    t = M.scan_instants(Tp / 4.0, Tp, 64)
    (dmin, tmin, ins, ent), _, _ = M.scan_relative(t, *path(t), R)
    assert (ins, ent) == (1, 1) and tmin == Tp / 4.0
    t = M.scan_instants(0.0, Tp, 100)
    assert M.scan_relative(t, *path(t), R)[0][2:] == (0, 2)
    t = M.scan_instants(0.0, Tp, 2)                                       # each half holds one dip
    assert M.scan_relative(t, *path(t), R)[0][2:] == (0, 2)
    t = M.scan_instants(0.0, Tp, 1)
    assert M.scan_relative(t, *path(t), R)[0][3] <= 1


def test_counts_and_out_restated():
    samples = np.zeros((2, 6, M.NMS))
    samples[0, :, 2] = [1, 0, 0, 0, 1, 0]; samples[0, :, 3] = [0, 2, 0, 1, 1, 0]; samples[0, 5, 4] = 1.0; samples[0, 5, 3] = 7.0
    samples[1, :, 4] = 2.0
    cn = M.counts_of(samples)
    assert cn.tolist() == [[6, 1, 2, 4, 1 + 4 + 0 + 1 + 4, 4], [6, 6, 0, 0, 0, 0]]
    out = M.out_of(cn[:1], [10.0], [20.0])
    b = np.array([1.0, 2.0, 0.0, 1.0, 2.0])
    assert np.allclose(out[0], [0.8, np.sqrt(0.8 * 0.2 / 5), 0.4, 0.8, np.sqrt(b.var(ddof=1) / 5), 0.4, 10.0, 20.0, 5.0], rtol=1e-14)


def test_cumulative_joins_worlds_not_probabilities():
    """two events of one pair that hit in the SAME worlds: the joint fraction is that of one event, not 1 - (1 - p)^2"""
    N = 8
    samples = np.zeros((3, N, M.NMS))
    samples[0, :4, 3] = 1.0; samples[1, :4, 2] = 1.0; samples[2, 6, 3] = 2.0
    samples[1, 7, 4] = 1.0                                             # a failed flight in the pair's second event: the world is left out
    out = np.zeros((3, _ffi.NMC))
    res = cj.MonteCarloCollisionResult(np.zeros((3, 4)), out, np.zeros((3, 6), dtype=np.int64), np.zeros(3, dtype=I32), samples=samples)
    ev = cj.EncounterEvents(np.zeros((3, 2, 4)), np.zeros((3, 2, 2), dtype=I32), [2, 1, 0], [0, 0, 0])
    p, se = res.cumulative(ev)
    assert np.allclose(p, [4.0 / 7.0, 1.0 / 8.0, 0.0]) and np.allclose(se[:2], np.sqrt(p[:2] * (1.0 - p[:2]) / np.array([7.0, 8.0]))) and se[2] == 0.0
    indep = cj.cumulative_probability(ev, np.array([0.5, 0.5, 0.125]))
    assert indep[0] == 0.75 and p[0] < indep[0]
    res.status[1] = 6
    assert np.isnan(res.cumulative(ev)[0][0])
    with pytest.raises(ValueError, match="return_samples"):
        cj.MonteCarloCollisionResult(np.zeros((3, 4)), out, np.zeros((3, 6), dtype=np.int64), np.zeros(3, dtype=I32)).cumulative(ev)


# ---------------------------------------------------------------- the wrappers
S, N, D, NC = 3, 5, 2, 4


def ramp(*shape, start=0.0):
    return start + 0.01 * np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape)


Y, U, UNITS, SPAN, CONSTS = ramp(S, 7, N, start=1.0), ramp(S, 3, N, start=2.0), ramp(S, 2, start=3.0), ramp(S, 2, start=4.0), ramp(S, 8, start=5.0)
P0 = ramp(6, 6, start=7.0)
CY, CUNITS, CSPAN, CCONSTS, CP0 = ramp(D, 7, NC, start=8.0), ramp(D, 2, start=9.0), ramp(D, 2, start=10.0), ramp(D, 8, start=11.0), ramp(D, 6, 6, start=12.0)
NS, CNS, RADIUS, CRADIUS = [5, 4, 3], [4, 3], [1.0, 2.0, 3.0], [4.0, 5.0]
PAIRS = f64([[0, 1, 100.0, 20.0], [2, 0, 200.0, 30.0], [1, 0, 300.0, 40.0]])
HALF, EXEC, MVAR, ATMO = [10.0, 20.0, 30.0], ramp(5, start=13.0), [0.1, 0.2, 0.3], f64([1.0, 2.0, 3.0, 4.0])
BLOCKS = [(0, 2), (2, 1)]


@pytest.fixture
def mc_rec(rec, monkeypatch):
    monkeypatch.setattr(_ffi, "lptr", lambda a: a)
    return rec


def mc_want(ctx, rows, half, full, NSAMP, outputs):
    c = len(rows)
    NSl = 1 if full else 2
    flags = _ffi.FLAG_DRAG | _ffi.FLAG_J2 | _ffi.FLAG_ATMO if full else 0
    return [ctx, c, rows, S, N, i32(NS) if full else None, Y, U if full else None, UNITS, SPAN, CONSTS, flags, 2e-3 if full else cj.DEFAULT_PROP_MAX_STEP,
            np.broadcast_to(P0, (S, 6, 6)), np.broadcast_to(EXEC, (S, 5)) if full else None, f64(MVAR) if full else None, f64(RADIUS)] \
        + ([D, NC, i32(CNS), CY, CUNITS, CSPAN, CCONSTS, CP0, f64(CRADIUS)] if full else [0, 0] + [None] * 7) \
        + [f64(half), 100 if full else 64, NSAMP, (1 << 63) + 5 if full else 0, 4096 if full else 0, Out(c, _ffi.NMCC, dtype=np.int64, zero=True),
           Out(c, _ffi.NMC), Out(c, dtype=I32, zero=True)] \
        + ([Out(c, NSAMP, _ffi.NMS), Out(c, NSl, NSAMP, 7, N), Out(c, NSl, NSAMP, 3, N)] if outputs else [None] * 3)


@pytest.mark.parametrize("devices", [None, [0, 0]])
@pytest.mark.parametrize("full", [False, True])
def test_wrapper_marshalling(mc_rec, full, devices):
    """the plain call (all-pairs, no thrust, no execution errors, no optional outputs) and the full one (catalogue, node counts,
    thrust, execution, mass variance, model, seed above 2^63, scan, max_flights, every optional output), on one context and on
    devices=[0, 0]: blocks of 2 and 1 rows of the list and of half_window, the whole of everything else, written in place"""
    NSAMP = 7
    kw = dict(seed=(1 << 63) + 5, scan=100, execution=EXEC, mass_var0=MVAR, ns=NS, cat=(CY, CUNITS, CSPAN, CCONSTS, CP0, CRADIUS, CNS),
              include_drag=True, include_J2=True, atmosphere=ATMO, prop_max_step=2e-3, max_flights=4096, return_samples=True,
              return_trajectories=True) if full else {}
    res = cj.collision_probability_mc(PAIRS, RADIUS, Y, U if full else None, UNITS, SPAN, CONSTS, P0, HALF, NSAMP, devices=devices, **kw)
    calls = mc_rec.named("mpcx_collision_probability_mc")
    blocks = BLOCKS if devices else [(0, 3)]
    assert len(calls) == len(blocks)
    for slot, (call, (first, count)) in enumerate(zip(calls, blocks)):
        blk = slice(first, first + count)
        args = check_call(call, "mpcx_collision_probability_mc", mc_want(("ctx", 0, slot), PAIRS[blk], HALF[blk], full, NSAMP, full))
        for i, arr in ((31, res.counts), (33, res.status)) + (((34, res.samples), (35, res.Y_samples), (36, res.U_samples)) if full else ()):
            assert np.shares_memory(args[i], arr[blk]) and args[i].shape == arr[blk].shape
        assert np.shares_memory(args[32], res.p_hit)
    assert res.p_hit.shape == (3,) and res.window.shape == (3, 2) and res.counts.dtype == np.int64
    assert (res.samples is None) == (not full)
    if full:
        assert mc_rec.named("mpcx_set_atmosphere")


def test_wrapper_checks_and_the_empty_list(mc_rec):
    empty = cj.collision_probability_mc(np.zeros((0, 4)), RADIUS, Y, None, UNITS, SPAN, CONSTS, P0, 5.0, 9, return_samples=True)
    assert not mc_rec.calls and empty.p_hit.shape == (0,) and empty.samples.shape == (0, 9, _ffi.NMS) and empty.counts.shape == (0, 6)
    good = dict(pairs=PAIRS, radius=RADIUS, Y=Y, U=U, units=UNITS, span=SPAN, consts=CONSTS, P0=P0, half_window=HALF, samples=4)
    for change, message in [(dict(samples=0), "samples: need an integer >= 1"), (dict(samples=2.5), "samples"), (dict(scan=0), "scan: need an integer >= 1"),
                            (dict(seed=-1), "seed"), (dict(seed=1 << 64), "seed"), (dict(max_flights=-1), "max_flights"),
                            (dict(prop_max_step=0.0), "max_step"), (dict(P0=np.eye(5)), "P0"), (dict(execution=np.zeros(4)), "execution"),
                            (dict(mass_var0=[1.0, 2.0]), "mass_var0"), (dict(half_window=[1.0, 2.0]), "half_window"),
                            (dict(U=np.zeros((S, 3, N + 1))), "U: expected"), (dict(radius=None), "radius"),
                            (dict(cat=(CY, CUNITS, CSPAN, CP0, CRADIUS)), "cat: expected"),
                            (dict(cat=(CY, CUNITS, CSPAN, CCONSTS[:1], CP0, CRADIUS)), "cat_consts"),
                            (dict(pairs=np.zeros((2, 3))), "pairs")]:
        with pytest.raises(ValueError, match=message):
            cj.collision_probability_mc(**{**good, **change})
    assert not mc_rec.calls


def test_binding_constants_match_the_header():
    import os
    import re
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mpcx.h")).read()
    for name, val in (("NMCC", _ffi.NMCC), ("NMC", _ffi.NMC), ("NMS", _ffi.NMS)):
        assert int(re.search(rf"#define MPCX_{name} (\d+)", txt).group(1)) == val
    for prefix, names in (("MCC", ["FLOWN", "FAILED", "START", "ENTRIES", "SQUARES", "HIT"]),
                          ("MC", ["P_HIT", "SE_HIT", "START", "ENTRIES", "SE_BOUND", "EXCESS", "TA", "TB", "N_OK"]),
                          ("MS", ["DMIN", "T_MIN", "INSIDE_START", "ENTRIES", "STATUS"])):
        order = re.findall(rf"MPCX_{prefix}_([A-Z_]+?)\b(?: = 0)?[,; }}]", txt[txt.index(f"enum {{ MPCX_{prefix}_"):][:600])
        assert order[:len(names)] == names, (prefix, order)
        assert [getattr(_ffi, f"{prefix}_{n}") for n in names] == list(range(len(names)))
    import mpconstellation_amd as pkg
    assert pkg.collision_probability_mc is cj.collision_probability_mc and pkg.MonteCarloCollisionResult is cj.MonteCarloCollisionResult
    assert "collision_probability_mc" in pkg.__all__ and "MonteCarloCollisionResult" in pkg.__all__


def test_constellation_mpc_hands_the_plan_to_both_calls(monkeypatch):
    """ConstellationMPC.collision_probability_mc: the plan is screened, the window call gets plan_covariance(P0, execution, mass_var0)
    without noise, the Monte Carlo call the same rows, plan, thrust, P0, execution and the model's keywords"""
    from mpconstellation_amd import ConstellationMPC
    mpc = ConstellationMPC.__new__(ConstellationMPC)
    seen = {}
    w = dict(Y="Y", ns="ns", units="units", span="span", M=9, T0=0.0, T1=1.0)
    monkeypatch.setattr(mpc, "_plan_probabilities", lambda *a: (seen.setdefault("plan", a), (w, "screened", "P", dict(ns="ns", cat=None, device=1, devices=None)))[1],
                        raising=False)
    mpc._plan, mpc.consts = ("X", "Uplan"), "consts"
    mpc.plan_drag, mpc.plan_J2, mpc.include_drag, mpc.include_J2, mpc.atmosphere = False, True, True, True, "atmo"
    monkeypatch.setattr(cj, "collision_probability_window", lambda *a, **k: seen.setdefault("window", (a, k)) and "W")
    monkeypatch.setattr(cj, "collision_probability_mc", lambda *a, **k: seen.setdefault("mc", (a, k)) and "MC")
    out = mpc.collision_probability_mc(500.0, "P0", 2.0, 60.0, 1000, seed=3, execution="ex", mass_var0="mv", scan=32, model="truth", max_flights=77)
    assert out == ("screened", "W", "MC")
    assert seen["plan"] == (500.0, "P0", None, 4, None, None, "ex", "mv")
    assert seen["window"] == (("screened", 2.0, "Y", "units", "span", "P", 60.0), dict(panels=4, ns="ns", device=1, devices=None))
    a, k = seen["mc"]
    assert a == ("screened", 2.0, "Y", "Uplan", "units", "span", "consts", "P0", 60.0, 1000)
    assert k == dict(seed=3, scan=32, execution="ex", mass_var0="mv", prop_max_step=1e-3, max_flights=77, return_samples=False, return_trajectories=False,
                     include_drag=True, include_J2=True, atmosphere="atmo", ns="ns", device=1, devices=None)
