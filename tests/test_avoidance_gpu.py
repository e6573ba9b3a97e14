"""Avoidance manoeuvres on the device (csrc/avoidance.hip) against their numpy restatement (avoidance_reference.py) fed the device's
own A, B_kn, B_kp, against themselves (same bits across forms, with and without sens, across contexts), and end to end: a planted
encounter screened, opened to 4 sigma, flown again and screened again.

Tolerances, from the arithmetic (avoidance_reference.avoidance, with_bounds=True): the sensitivities get the product bound along
the sweep with gamma = 32 eps (in the manner of collision_reference.chain_error_bound) started from the seeds' error -- positions of
7e6 m through the Hermite differ by about 2e-7 m (test_collision_gpu.py), which turns the frame by 4e-7 / |m|; du and out are smooth
functions of the sensitivities, the miss and W, and get that relative error times cond(M) cond(W)."""
import functools

import numpy as np
import pytest

import avoidance_reference as AR
import collision_reference as C
import conjunction_reference as R

pytestmark = pytest.mark.gpu


def scale_constants(lengths):
    from mpconstellation_amd.satellite_scale import SatelliteScale
    return np.stack([SatelliteScale(x=np.array([L, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])).get_normalized_constants().as_vector() for L in lengths])


def device_stage(X, U, units, span, consts, ns=None, flags=0):
    """the device's own A (S, K-1, 7, 7), B_kn, B_kp (S, K-1, 7, 3) from the existing mpcx_discretize_batch about (X, U, tf); a ragged
    batch takes every count's satellites through a plain launch of that length (as test_collision_gpu.py::restated_chain does)"""
    from mpconstellation_amd import _ffi, conjunction as cj
    S, _, K = X.shape
    tf = (span[:, 1] - span[:, 0]) / units[:, 1]
    A, Bn, Bp = np.zeros((S, K - 1, 7, 7)), np.zeros((S, K - 1, 7, 3)), np.zeros((S, K - 1, 7, 3))
    counts = np.full(S, K) if ns is None else ns
    for nn in np.unique(counts):
        at = np.flatnonzero(counts == nn)
        x, u = _ffi.as_f64(X[at][:, :, :nn]), _ffi.as_f64(U[at][:, :, :nn])
        n = len(at) * (nn - 1)
        a, bp, bn, sg, xi = np.empty((len(at), nn - 1, 7, 7)), np.empty((len(at), nn - 1, 7, 3)), np.empty((len(at), nn - 1, 7, 3)), np.empty(n * 7), np.empty(n * 7)
        st = np.zeros(len(at), dtype=np.int32)
        _ffi.call("mpcx_discretize_batch", _ffi.context(0), len(at), int(nn), int(nn), _ffi.dptr(x), _ffi.dptr(u), _ffi.dptr(_ffi.as_f64(tf[at])),
                  _ffi.dptr(_ffi.as_f64(consts[at])), flags, cj.DEFAULT_MAX_STEP, _ffi.dptr(a), _ffi.dptr(bp), _ffi.dptr(bn), _ffi.dptr(sg), _ffi.dptr(xi),
                  _ffi.iptr(st))
        assert (st == 0).all()
        A[at, :nn - 1], Bn[at, :nn - 1], Bp[at, :nn - 1] = a, bn, bp
    return A, Bn, Bp


@functools.lru_cache(maxsize=None)
def scene(S, K, n, ragged):
    """S thrusting satellites on random circular LEO orbits (rows of K nodes over 3000 s; ragged: counts between 2 and K, the first is
    2, 1e300 behind them; the mass row falls by 10 % along the arc) and a catalogue of n objects with rows of the same length, object
    j on a circular orbit that passes satellite i_j's interpolated position at t_j within 50 .. 500 m at a crossing angle of 0.5 ..
    2.6 rad; t_j on a node of the satellite (not the first) for even j, anywhere for odd j.  Random covariances at every node.
    -> dict: rows = (Y, units, span, ns), U, consts, P, cat = (Y, units, span, ns, P), pairs (n, 4).  Treat as read-only."""
    rng = np.random.default_rng(1000 + 31 * S + 7 * K + n + (500 if ragged else 0))
    orb = R.random_orbits(S, seed=3 + S + K)
    span_rows = (-1.0, 2999.0)
    Y, units, span = R.trajectories(orb, K, span_rows)
    ns = None
    if ragged:
        ns = rng.integers(2, K + 1, S).astype(np.int32)
        ns[0] = 2
        for s in range(S):
            Ys, _, _ = R.trajectories({k: v[s:s + 1] for k, v in orb.items()}, int(ns[s]), span_rows)
            Y[s] = 1e300
            Y[s, :, :ns[s]] = Ys[0]
    counts = np.full(S, K) if ns is None else ns
    U = np.full((S, 3, K), 1e300)
    for s in range(S):
        Y[s, 6, :counts[s]] = 1.0 - 0.1 * np.arange(counts[s]) / K
        U[s, :, :counts[s]] = 0.02 * rng.standard_normal((3, counts[s]))
    side = (Y, units, span, np.zeros((S, K, 6, 6)), np.zeros(S), ns)
    cY = np.full((n, 7, K), np.nan); cunits = np.empty((n, 2)); cspan = np.empty((n, 2)); cns = np.empty(n, dtype=np.int32)
    pairs = np.empty((n, 4))
    for j in range(n):
        i = int(rng.integers(S))
        hn = (span[i, 1] - span[i, 0]) / (counts[i] - 1)
        t = span[i, 0] + hn * int(rng.integers(1, counts[i])) if j % 2 == 0 else float(rng.uniform(span[i, 0] + 30.0, span[i, 1] - 30.0))
        st, p, v, _, _ = C.state_and_cov_at(side, float(i), t, C.MU_EARTH)
        assert st == 0
        e = rng.normal(size=3); e /= np.linalg.norm(e)
        miss = float(rng.uniform(50.0, 500.0))
        q = p + miss * e
        qh = q / np.linalg.norm(q)
        vh = v - (v @ qh) * qh; vh /= np.linalg.norm(vh)
        ang = float(rng.uniform(0.5, 2.6))
        vhat = np.cos(ang) * vh + np.sin(ang) * np.cross(qh, vh)
        cns[j] = max(2, K - 3) if j % 2 else K
        cspan[j] = (float(rng.uniform(-50.0, -5.0)), float(rng.uniform(3005.0, 3050.0)))
        cY[j, :, :cns[j]], cunits[j] = C.circular_through(q, vhat, t, int(cns[j]), cspan[j])
        pairs[j] = (i, j, miss, t)
    return dict(rows=(Y, units, span, ns), U=U, consts=scale_constants(units[:, 0]), P=C.random_covariances(rng, S, K),
                cat=(cY, cunits, cspan, cns, C.random_covariances(rng, n, K)), pairs=pairs)


def union_of(sc):
    """the scene as ONE constellation [satellites; catalogue] (the objects fly without thrust, the NaN behind their counts made
    finite for the discretiser's launch of full rows) and its list with j moved behind the satellites: the all-pairs form"""
    (Y, units, span, ns), (cY, cunits, cspan, cns, cP) = sc["rows"], sc["cat"]
    S, K = Y.shape[0], Y.shape[2]
    counts = np.full(S, K, dtype=np.int32) if ns is None else ns
    rows = (np.concatenate([Y, cY]), np.concatenate([units, cunits]), np.concatenate([span, cspan]), np.concatenate([counts, cns]))
    U = np.concatenate([sc["U"], np.zeros((len(cY), 3, K))])
    consts = np.concatenate([sc["consts"], scale_constants(cunits[:, 0])])
    pairs = sc["pairs"].copy(); pairs[:, 1] += S
    return dict(rows=rows, U=U, consts=consts, P=np.concatenate([sc["P"], cP]), pairs=pairs)


def run(sc, target, who="i", P=False, cat=True, sens=True, pairs=None, **kw):
    from mpconstellation_amd import avoidance
    Y, units, span, ns = sc["rows"]
    c = None
    if cat:
        cY, cunits, cspan, cns, cP = sc["cat"]
        c = (cY, cunits, cspan, cP, cns) if P else (cY, cunits, cspan, cns)
    return avoidance(sc["pairs"] if pairs is None else pairs, target, Y, sc["U"], units, span, sc["consts"], ns=ns, P=sc["P"] if P else None, cat=c,
                     who=who, return_sensitivities=sens, **kw)


def restated(sc, stage, target, who="i", P=False, cat=True, pairs=None):
    c = None
    if cat:
        cY, cunits, cspan, cns, cP = sc["cat"]
        c = (cY, cunits, cspan, cns, cP if P else None)
    return AR.avoidance(sc["pairs"] if pairs is None else pairs, sc["rows"], stage, target, who, P=sc["P"] if P else None, cat=c, with_bounds=True)


def assert_within(res, ref, what):
    out, du, sens, status, (Eo, Ed, Es) = ref
    assert np.array_equal(res.status, status) and (status == 0).all(), (res.status, status)
    worst = {}
    for name, got, want, E in (("sens", res.sens, sens, Es), ("du", res.du, du, Ed), ("out", res.out, out, Eo)):
        d = np.abs(got - want)
        worst[name] = float((d / np.where(E > 0.0, E, 1.0)).max())
        assert np.isfinite(got).all() and (d <= E).all(), (what, name, worst[name])
    print(f"{what}: worst |device - restated| / bound: sens {worst['sens']:.3e}, du {worst['du']:.3e}, out {worst['out']:.3e}")


CASES = [(1, 2, 2, False), (3, 5, 3, False), (65, 5, 30, False), (65, 2, 30, True), (3, 2, 30, False)]


@pytest.mark.parametrize("n,S,K,ragged", CASES)
def test_device_against_the_restatement(n, S, K, ragged):
    """sens, du and out within the entrywise bounds computed from the inputs, in the catalogue form with a target in metres and with a
    Mahalanobis target, and in the all-pairs form of the union with both objects or object j manoeuvring"""
    sc = scene(S, K, n, ragged)
    Y, units, span, ns = sc["rows"]
    # rows of 2 or 3 nodes over 3000 s interpolate a circle so badly that the "planted" pairs are up to 1e6 m (3e3 sigma) apart:
    # the targets are beyond that, so that those rows manoeuvre too
    T_m, T_s = (1000.0, 6.0) if K >= 30 else (1.0e7, 1.0e5)
    what = f"n {n} S {S} K {K} ragged {ragged}"
    stage = device_stage(Y, sc["U"], units, span, sc["consts"], ns)
    assert_within(run(sc, T_m), restated(sc, stage, T_m), what + ", catalogue, metres")
    assert_within(run(sc, T_s, P=True), restated(sc, stage, T_s, P=True), what + ", catalogue, Mahalanobis")
    un = union_of(sc)
    uY, uunits, uspan, uns = un["rows"]
    ustage = device_stage(np.nan_to_num(uY, nan=1.0), un["U"], uunits, uspan, un["consts"], uns)
    both = run(un, T_s, who="both", P=True, cat=False)
    assert_within(both, restated(un, ustage, T_s, "both", P=True, cat=False), what + ", all pairs, both move, Mahalanobis")
    res_j = run(un, T_m, who="j", cat=False)
    assert_within(res_j, restated(un, ustage, T_m, "j", cat=False), what + ", all pairs, j moves, metres")
    assert not res_j.du[:, 0].any() and not res_j.sens[:, 0].any() and not res_j.dv[:, 0].any() and res_j.du[:, 1].any()
    assert (both.d0 < T_s).all() and both.du[:, 0].any() and both.du[:, 1].any()


def bits(r):
    return (r.out.tobytes(), r.du.tobytes(), r.status.tobytes())


def test_same_bits():
    """sens given or not; the catalogue form against the all-pairs form of the union with who='i'; two contexts against one; and with
    both objects moving the two thrust changes together displace the miss by (DM1, DM2)"""
    sc = scene(5, 30, 65, False)
    a = run(sc, 6.0, P=True)
    b = run(sc, 6.0, P=True, sens=False)
    assert (a.status == 0).all() and b.sens is None and bits(a) == bits(b)
    un = union_of(sc)
    c = run(un, 6.0, P=True, cat=False)
    assert np.array_equal(a.out, c.out) and np.array_equal(a.du[:, 0], c.du[:, 0]) and np.array_equal(a.sens[:, 0], c.sens[:, 0])
    assert not c.du[:, 1].any() and not c.sens[:, 1].any() and np.array_equal(a.status, c.status)
    d = run(sc, 6.0, P=True, devices=[0, 0])
    assert bits(a) == bits(d) and np.array_equal(a.sens, d.sens)
    e = run(un, 6.0, who="both", P=True, cat=False)
    f = run(un, 6.0, who="both", P=True, cat=False, sens=False, devices=[0, 0])
    assert (e.status == 0).all() and bits(e) == bits(f)
    uY, uunits, uspan, uns = un["rows"]
    ref = restated(un, device_stage(np.nan_to_num(uY, nan=1.0), un["U"], uunits, uspan, un["consts"], uns), 6.0, "both", P=True, cat=False)
    moved = np.einsum("nsrcm,nscm->nr", e.sens, e.du)                    # sum over both objects and all nodes of g_m du_m
    Edm = ref[4][0][:, AR.DM1:AR.DM2 + 1]
    print(f"both move: worst |sum g du - dm| / bound {np.max(np.abs(moved[:, :2] - e.dm) / Edm):.3e}; share of object i in dv "
          f"{np.min(e.dv[:, 0] / e.dv.sum(axis=1)):.3f} .. {np.max(e.dv[:, 0] / e.dv.sum(axis=1)):.3f}")
    assert (np.abs(moved[:, :2] - e.dm) <= Edm).all() and (e.dv > 0.0).all()
    assert (np.abs(-moved[:, 2] / np.array([AR.frame(*_rel(un, r))[4] for r in un["pairs"]]) - e.dt) <= ref[4][0][:, AR.DT]).all()


def _rel(sc, row):
    """relative position and velocity of a pair of the all-pairs form at its time"""
    Y, units, span, ns = sc["rows"]
    side = (Y, units, span, np.zeros((len(Y), Y.shape[2], 6, 6)), np.zeros(len(Y)), ns)
    _, pa, va, _, _ = C.state_and_cov_at(side, row[0], row[3], C.MU_EARTH)
    _, pb, vb, _, _ = C.state_and_cov_at(side, row[1], row[3], C.MU_EARTH)
    return pb - pa, vb - va


def scene_with_zero_miss(n):
    """collision_reference.encounter_scene(n) and one more catalogue object that is WHERE its satellite is at the pair's time: it has
    the satellite's units, span and node count, the time is one at which both Hermite parameters are exactly 0 -- (t - ta) / hn an
    integer in floating point, so that both positions are the node's own product y L -- and its position row at that node is the
    satellite's; it crosses at 1 rad.  The miss of that pair is exactly 0: the frame's e_1 comes from the fallback on the smallest
    axis.  -> rows, cat = (Y, units, span, P, radius, ns), pairs (n + 1, 4)"""
    base = C.encounter_scene(n)
    (Y, units, span, P, radius, _), (cY, cunits, cspan, cP, cradius, cns) = base["rows"], base["cat"]
    K, i = Y.shape[2], 2
    ta, L, Tu = span[i, 0], units[i, 0], units[i, 1]
    hn = (span[i, 1] - ta) / float(K - 1)                               # (cp_state's expressions)
    k, t = next((k, t) for k in range(K // 2, K - 2) for t in np.nextafter(ta + k * hn, [-np.inf, np.inf, 0.0]).tolist() + [ta + k * hn]
                if (t - ta) / hn == float(k))
    p, v = Y[i, :3, k] * L, Y[i, 3:6, k] * (L / Tu)
    ph = p / np.linalg.norm(p)
    vh = v - (v @ ph) * ph; vh /= np.linalg.norm(vh)
    y, (Lo, To) = C.circular_through(p, np.cos(1.0) * vh + np.sin(1.0) * np.cross(ph, vh), t, K, span[i])
    y[:3] *= Lo / L; y[3:6] *= (Lo / To) / (L / Tu)                     # in the satellite's units
    y[:3, k] = Y[i, :3, k]
    rng = np.random.default_rng(77)
    cat = (np.concatenate([cY, y[None]]), np.concatenate([cunits, units[i:i + 1]]), np.concatenate([cspan, span[i:i + 1]]),
           np.concatenate([cP, C.random_covariances(rng, 1, K)]), np.append(cradius, 5.0), np.append(cns, K).astype(np.int32))
    return base["rows"], cat, np.concatenate([base["pairs"], [[i, n, 0.0, t]]])


def test_one_encounter_across_calls():
    """collision_probability, avoidance and avoidance_joint run ONE encounter frame (collision_device.hpp): on the same list, with a
    target in metres, the miss of the first, D0 of the second and d0 of the third have the same bits -- the pair with a miss of
    exactly 0 included -- and the speed the first reports is the |w| the second divides by in DT = -sum_m g_m[e_w] . du_m / |w|.
    That sum is the device's butterfly over the nodes and numpy's here: the two differ by at most (3 K + 2) eps sum |terms| (the bound
    of a floating-point sum of 3 K terms in any order, and the products), the division adds 2 eps |DT|."""
    from mpconstellation_amd import _ffi, avoidance, avoidance_joint, collision_probability
    rows, cat, pairs = scene_with_zero_miss(7)
    Y, units, span, P, radius, _ = rows
    cY, cunits, cspan, cP, cradius, cns = cat
    S, _, K = Y.shape
    U, consts = np.zeros((S, 3, K)), scale_constants(units[:, 0])
    cp = collision_probability(pairs, radius, Y, units, span, P, cat=cat)
    av = avoidance(pairs, 1000.0, Y, U, units, span, consts, cat=(cY, cunits, cspan, cns), return_sensitivities=True)
    aj = avoidance_joint(pairs, 1000.0, Y, U, units, span, consts, cat=(cY, cunits, cspan, cns))
    print("miss", cp.miss, "speed", cp.speed, "statuses", cp.status, av.status, aj.row_status, aj.status)
    assert len(pairs) == 8 and not cp.status.any() and not av.status.any() and not aj.row_status.any()
    assert cp.miss[-1] == 0.0 and (cp.miss[:-1] > 0.0).all()
    assert cp.miss.tobytes() == av.out[:, _ffi.AV_D0].tobytes() == aj.d0.tobytes()
    terms = av.sens[:, 0, 2] * av.du[:, 0]                                # (n, 3, K): the e_w row of g_m times du_m
    eps = np.finfo(np.float64).eps
    bound = (3 * K + 2) * eps * np.abs(terms).sum(axis=(1, 2)) / cp.speed + 2 * eps * np.abs(av.dt)
    worst = np.abs(-terms.sum(axis=(1, 2)) / cp.speed - av.dt) / bound
    print(f"DT against -sum g_w du / speed: worst difference / bound {worst.max():.3e}")
    assert av.du.any(axis=(1, 2, 3)).all() and (worst <= 1.0).all()


def test_statuses_in_one_call():
    """good, t past a span (BADK), j out of range (BADK), t exactly at the first node (SINGULAR: nothing before it to thrust with),
    already beyond the target (OK, du = 0, D1 = D0): failed rows all NaN, the good rows the bits of a call without the bad ones"""
    sc = scene(5, 30, 65, False)
    Y, units, span, ns = sc["rows"]
    union = union_of(sc)
    misses = np.array([AR.frame(*_rel(union, r))[3] for r in union["pairs"]])      # in the encounter plane: what d0 is with W = I
    near, far = np.flatnonzero(misses < 250.0)[:3], np.flatnonzero(misses > 320.0)[0]
    rows = sc["pairs"][[near[0], near[1], near[2], near[0], far]].copy()
    rows[1, 3] = 1.0e6                                                   # outside both spans
    rows[2, 1] = len(sc["cat"][0])                                       # no such object
    rows[3, 3] = span[int(rows[3, 0]), 0]                                # the satellite's first node (the object's span starts earlier)
    res = run(sc, 300.0, pairs=rows)
    print("statuses", res.status, "d0", res.d0, "d1", res.d1)
    assert res.status.tolist() == [0, AR.ST_BADK, AR.ST_BADK, AR.ST_SINGULAR, 0]
    for r in (1, 2, 3):
        assert np.isnan(res.out[r]).all() and np.isnan(res.du[r]).all() and np.isnan(res.sens[r]).all()
    for r in (0, 4):
        assert np.isfinite(res.out[r]).all() and np.isfinite(res.du[r]).all() and np.isfinite(res.sens[r]).all()
    assert res.d0[0] < 300.0 and abs(res.d1[0] - 300.0) < 1e-6 and res.du[0].any()
    assert res.d0[4] > 300.0 and res.d1[4] == res.d0[4] and not res.du[4].any() and res.sens[4].any() and not res.out[4, AR.DM1:AR.DT + 1][[0, 1, 3]].any()
    assert res.miss1[4] == res.d0[4] and not res.dv[4].any() and not res.umax[4].any()
    alone = run(sc, 300.0, pairs=rows[[0, 4]])
    assert np.array_equal(alone.out, res.out[[0, 4]]) and np.array_equal(alone.du, res.du[[0, 4]]) and np.array_equal(alone.sens, res.sens[[0, 4]])


def test_c_abi_refuses_bad_arguments():
    from mpconstellation_amd import _ffi
    lib, ctx = _ffi.load(), _ffi.context(0)
    S, K, n = 2, 5, 3
    Y, U, units, span, consts = np.ones((S, 7, K)), np.zeros((S, 3, K)), np.ones((S, 2)), np.array([[0.0, 1.0]] * S), np.ones((S, 8))
    P = np.zeros((S, K, 6, 6))
    pairs, out, du, st = np.zeros((n, 4)), np.zeros((n, _ffi.NAV)), np.zeros((n, 2, 3, K)), np.zeros(n, dtype=np.int32)
    d, i = _ffi.dptr, _ffi.iptr
    none = (0, 0, None, None, None, None, None)
    cat = (S, K, None, d(Y), d(units), d(span), None)

    def av(n=n, S=S, K=K, flags=0, max_step=1e-2, P=None, cols=none, mu=C.MU_EARTH, target=10.0, who=0):
        return lib.mpcx_avoidance(ctx, n, d(pairs), S, K, None, d(Y), d(U), d(units), d(span), d(consts), flags, max_step, P, *cols, mu, target, who,
                                  d(out), d(du), None, i(st))
    for bad in (dict(n=0), dict(S=0), dict(K=1), dict(mu=0.0), dict(target=0.0), dict(target=np.inf), dict(target=np.nan), dict(who=3), dict(who=-1),
                dict(flags=4), dict(flags=_ffi.FLAG_ATMO), dict(max_step=0.0), dict(cols=cat, who=1), dict(cols=cat, who=2), dict(cols=cat, P=d(P)),
                dict(cols=(0, K) + cat[2:]), dict(cols=(S, 1) + cat[2:])):
        assert av(**bad) == -2, bad
        assert b"avoidance" in lib.mpcx_last_error(ctx) or b"ATMO" in lib.mpcx_last_error(ctx)
    w = lib.mpcx_avoidance_workspace_bytes
    assert w(0, 2, 5) == 0 and w(3, 0, 5) == 0 and w(3, 2, 1) == 0 and w(3, 2, 5) >= 2 * 4 * _ffi.STAGE_DOUBLES * 8 + 3 * 2 * 9 * 5 * 8


def arc_on_device(U):
    """the host tests' thrusting arc flown by propagate_batch under a CTRL_SEQUENCE law on its own K nodes: x (7, K)"""
    from mpconstellation_amd import _ffi, propagate_batch
    a = AR.arc_setup()
    K = AR.SCENE["K"]
    y, st, _ = propagate_batch(a["y0"][None], [AR.SCENE["tf"]], a["consts"][None], (_ffi.CTRL_SEQUENCE, U[None], K, 1.0), K, max_step=AR.SCENE["prop_max_step"])
    assert st.tolist() == [0]
    return y[0]


def test_end_to_end_planted_encounter():
    """The planted encounter of the host tests (200 m in the encounter plane, mid-interval) on the device: screen_against ->
    covariance of both -> avoidance(target = 4 sigma) -> apply -> propagate_batch again -> screen_against -> collision_probability.
    The Mahalanobis distance of the new encounter is held to the target within 1.43e-3 relative -- test_avoidance_host.py's
    MISS_BOUND = 10 x the 1.43e-4 it measured between the linear prediction and the nonlinear flow -- and the probability must fall."""
    from mpconstellation_amd import screen_against, covariance, collision_probability, avoidance
    from test_avoidance_host import MISS_BOUND
    a = AR.arc_setup()
    K = AR.SCENE["K"]
    x = arc_on_device(a["U"])
    sc = dict(a, x=x)
    hn = (a["span"][1] - a["span"][0]) / (K - 1)
    cy, cu, cspan = AR.planted_object(sc, a["span"][0] + 20.37 * hn)
    units, span, consts = a["units"][None], a["span"][None], a["consts"][None]
    cY, cunits, cspans = cy[None], cu[None], cspan[None]
    P0 = np.diag([40.0 ** 2] * 3 + [0.02 ** 2] * 3)
    cP = covariance(cY, cunits, cspans, scale_constants(cunits[:, 0]), P0)
    grid = dict(M=4 * (K - 1) + 1, T0=float(span[0, 0]), T1=float(span[0, 1]), threshold=5000.0)

    def assess(x, U):
        scr = screen_against(Y=x[None], units=units, span=span, cat_Y=cY, cat_units=cunits, cat_span=cspans, **grid)
        P = covariance(x[None], units, span, consts, P0, U=U[None])
        col = collision_probability(scr, 5.0, x[None], units, span, P, cat=(cY, cunits, cspans, cP, 5.0))
        return scr, P, col
    scr, P, col = assess(x, a["U"])
    assert scr.pairs[:, :2].tolist() == [[0.0, 0.0]] and col.status.tolist() == [0] and abs(col.miss[0] - 200.0) < 2.0
    av = avoidance(scr, 4.0, x[None], a["U"][None], units, span, consts, P=P, cat=(cY, cunits, cspans, cP))
    assert av.status.tolist() == [0] and abs(av.d0[0] - col.mahalanobis[0]) <= 1e-9 * av.d0[0] and abs(av.d1[0] - 4.0) <= 1e-9
    U2 = av.apply(a["U"][None], 0)[0]
    scr2, _, col2 = assess(arc_on_device(U2), U2)
    rel = abs(col2.mahalanobis[0] - 4.0) / 4.0
    print(f"before: miss {col.miss[0]:.2f} m, {col.mahalanobis[0]:.4f} sigma, Pc {col.pc[0]:.3e}; asked 4 sigma: dv {av.dv[0, 0]:.4f} m/s, umax {av.umax[0, 0]:.3e}, "
          f"DT {av.dt[0]:.4f} s (screen: {scr2.pairs[0, 3] - scr.pairs[0, 3]:.4f} s); after: miss {col2.miss[0]:.2f} m (predicted {av.miss1[0]:.2f}), "
          f"{col2.mahalanobis[0]:.6f} sigma ({rel:.3e} from the target), Pc {col2.pc[0]:.3e}")
    assert col2.status.tolist() == [0] and rel <= MISS_BOUND             # 1.43e-3
    assert col2.pc[0] < col.pc[0]


def test_constellation_mpc_avoidance():
    """five satellites, one update: the method returns what screen and conjunction.avoidance return on the plan, called by hand"""
    from mpconstellation_amd import Satellite, ConstellationMPC, conjunction as cj
    from mpconstellation_amd.constellation import constellation_states
    st = constellation_states(5)
    mpc = ConstellationMPC([Satellite(s[:3].copy(), s[3:6].copy(), float(s[6])) for s in st], base_res=30, tf_horizon=2, tf_interval=1, r_des=1.5)
    mpc.update()
    (w,) = mpc._screen_windows("plan", samples_per_node=4)
    for who, P0 in (("both", None), ("i", np.diag([100.0 ** 2] * 3 + [0.1 ** 2] * 3))):
        target = 1.0e8 if P0 is None else 1.0e6
        scr, av = mpc.avoidance(5.0e7, target, P0=P0, q=1e-8, who=who)
        scr2 = cj.screen(threshold=5.0e7, **w)
        P = None if P0 is None else cj.covariance(w["Y"], w["units"], w["span"], mpc.consts, P0, U=mpc._plan[1], ns=w["ns"], q=1e-8)
        av2 = cj.avoidance(scr2, target, w["Y"], mpc._plan[1], w["units"], w["span"], mpc.consts, ns=w["ns"], P=P, who=who)
        print(f"who {who}: {len(scr.pairs)} pairs, statuses {av.status}")
        ok = av.status == 0                                              # (a pair closest at the plan's first instant has nothing to thrust with)
        assert len(scr.pairs) == 10 and scr.pairs.tobytes() == scr2.pairs.tobytes() and ok.any()
        assert np.array_equal(av.out, av2.out, equal_nan=True) and np.array_equal(av.du, av2.du, equal_nan=True) and np.array_equal(av.status, av2.status)
        assert av.du.shape == (10, 2, 3, w["Y"].shape[2]) and (av.d1[ok] >= av.d0[ok]).all() and av.du[ok].any()
