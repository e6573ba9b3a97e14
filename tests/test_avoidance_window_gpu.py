"""Avoidance for slow encounters on the device (csrc/collision_window.hip: collision_window_sensitivity_kernel; csrc/
avoidance_window.hip) against the numpy restatement (avoidance_window_reference.py) fed the device's own A, B_kn, B_kp, against
themselves (same bits with and without the optional outputs, alone and in a list, across contexts), at their edges, and end to end:
a planted slow pair manoeuvred to a target two decades down, flown again, found again and measured again.

Tolerances, from the arithmetic (avoidance_window_reference): the state gradient gets twice collision_window_reference.
rounding_bound relative to the sum of its terms' magnitudes plus what the Hermite positions' 2e-7 m do through the factor z; the node
sources and the sweep get the product bound in the manner of avoidance_reference.sweep_error_bound; the step alpha is pinned by the
tolerance of the search over the slope of ln Q, and du, out follow it."""
import functools

import numpy as np
import pytest

import avoidance_reference as AR
import avoidance_window_reference as AW
import collision_reference as C
import collision_window_reference as CW

pytestmark = pytest.mark.gpu

TARGET, TOL, MAX_EVAL = 1e-6, 1e-6, 40


def scale_constants(lengths):
    from mpconstellation_amd.satellite_scale import SatelliteScale
    return np.stack([SatelliteScale(x=np.array([L, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])).get_normalized_constants().as_vector() for L in lengths])


def device_stage(X, U, units, span, consts, ns=None, flags=0):
    """the device's own A (S, K-1, 7, 7), B_kn, B_kp (S, K-1, 7, 3) from mpcx_discretize_batch about (X, U, tf), after
    test_avoidance_gpu.py's: a ragged batch takes every count's satellites through a plain launch of that length"""
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
def scene(K, S=5, rows_of=None):
    """collision_window_reference.window_scene(K) given a thrust table and constants as test_avoidance_gpu.py::scene makes them (the
    mass row falls by 10 % along the arc, U = 0.02 standard_normal, SatelliteScale constants), cut to the first S satellites and the
    rows `rows_of` (a tuple of row numbers; None: all 65), and its union [satellites; catalogue] for the all-pairs form.
    -> dict: rows, cat (sides as collision_window_reference takes them), U, consts, pairs, half and the same with a leading u for the
    union.  Treat as read-only."""
    sc = CW.window_scene(K)
    Y, units, span, P, radius, _ = sc["rows"]
    rng = np.random.default_rng(70 + K)
    Y = Y.copy()
    Y[:, 6, :] = 1.0 - 0.1 * np.arange(K) / K
    U = 0.02 * rng.standard_normal((len(Y), 3, K))
    consts = scale_constants(units[:, 0])
    sel = np.arange(len(sc["pairs"])) if rows_of is None else np.array(rows_of)
    assert (sc["pairs"][sel, 0] < S).all()
    rows = (Y[:S], units[:S], span[:S], P[:S], radius[:S], None)
    cat = sc["cat"]
    pairs, half = sc["pairs"][sel].copy(), sc["half"][sel].copy()
    cY, cunits, cspan, cP, cradius, cns = cat
    urows = (np.concatenate([rows[0], cY]), np.concatenate([rows[1], cunits]), np.concatenate([rows[2], cspan]), np.concatenate([rows[3], cP]),
             np.concatenate([rows[4], cradius]), np.concatenate([np.full(S, K, dtype=np.int32), cns]))
    upairs = pairs.copy(); upairs[:, 1] += S
    return dict(rows=rows, cat=cat, U=U[:S], consts=consts[:S], pairs=pairs, half=half, urows=urows, upairs=upairs,
                uU=np.concatenate([U[:S], np.zeros((len(cY), 3, K))]), uconsts=np.concatenate([consts[:S], scale_constants(cunits[:, 0])]))


@functools.lru_cache(maxsize=None)
def restated_gradients(K, S, rows_of, panels):
    """the state gradients of the scene's rows: they do not depend on the form or on who moves -> (catalogue form, union form)"""
    sc = scene(K, S, rows_of)
    g = AW.row_gradients(sc["pairs"], sc["rows"], sc["half"], panels, sc["cat"])
    gu = [dict(e, ob=None if e["ob"] is None else e["ob"] + S) for e in g]
    return g, gu


@functools.lru_cache(maxsize=None)
def stages(K, S, rows_of):
    sc = scene(K, S, rows_of)
    Y, units, span, _, _, _ = sc["rows"]
    uY, uunits, uspan, _, _, uns = sc["urows"]
    return (device_stage(Y, sc["U"], units, span, sc["consts"]),
            device_stage(np.nan_to_num(uY, nan=1.0), sc["uU"], uunits, uspan, sc["uconsts"], uns))


def run(sc, call, union=False, who="i", pairs=None, half=None, **kw):
    from mpconstellation_amd import conjunction as cj
    Y, units, span, P, radius, ns = sc["urows"] if union else sc["rows"]
    pr = (sc["upairs"] if union else sc["pairs"]) if pairs is None else pairs
    args = dict(radius=radius, Y=Y, U=sc["uU"] if union else sc["U"], units=units, span=span, consts=sc["uconsts"] if union else sc["consts"], P=P,
                half_window=sc["half"] if half is None else half, ns=ns, cat=None if union else sc["cat"], who=who, **kw)
    if call == "sens":
        return cj.collision_window_sensitivity(pr, **args)
    return cj.avoidance_window(pr, TARGET, tol=TOL, max_eval=MAX_EVAL, **args)


def window_bits(sc, union, panels, pairs=None, half=None):
    from mpconstellation_amd import collision_probability_window
    Y, units, span, P, radius, ns = sc["urows"] if union else sc["rows"]
    r = collision_probability_window((sc["upairs"] if union else sc["pairs"]) if pairs is None else pairs, radius, Y, units, span, P,
                                     sc["half"] if half is None else half, panels=panels, ns=ns, cat=None if union else sc["cat"])
    return np.column_stack([r.p, r.start, r.entries, r.rate_max, r.t_rate_max, r.window]), r.status


def sens_bits(r):
    out = np.column_stack([r.p, r.start, r.entries, r.rate_max, r.t_rate_max, r.window])
    return out.tobytes(), r.status.tobytes(), r.sens.tobytes()


CASES = [(2, 2, 1), (3, 5, 3), (30, 5, 65)]


def case_rows(K, S, n):
    """(1, 2, 2): the first slow row of the first two satellites -- its window of minutes is cut to the span of 100 s; (3, 5, 3): rows
    2, 3, 4 (slow, the same object twice, fast); (65, 5, 30): all, one row beyond a full block of 64"""
    sc = CW.window_scene(K)
    if n == 65:
        return None
    if n == 3:
        return (2, 3, 4)
    return (next(j for j in range(65) if j % 4 >= 2 and j != 3 and sc["pairs"][j, 0] < S),)


@pytest.mark.parametrize("panels", CW.SCENE_PANELS)
@pytest.mark.parametrize("K,S,n", CASES)
def test_device_against_the_restatement(K, S, n, panels):
    """Both calls within the entrywise bounds of the restatement fed the device's own stage records: the catalogue form (a ragged
    catalogue) and the all-pairs form of the union with who = i, j and both.  out of the sensitivity call has the bytes of
    collision_probability_window on the same inputs; state_grad is held to its own bound in every form.  The manoeuvre runs on the
    device in all four (form, who) combinations and is held to the restatement on the first eight rows of each (a km/s crossing,
    slow rows, the same object twice, ragged objects) and, in the catalogue form, on one more row of each class and on row 64 past
    the full block -- every restated evaluation is the full rule in numpy; on all rows the device's own P1 must be within tol of
    the target, and an object that does not move has du, DV and UMAX exactly 0.  EVALS is not compared: two correct searches may
    stop one evaluation apart."""
    rows_of = case_rows(K, S, n)
    sc = scene(K, S, rows_of)
    assert len(sc["pairs"]) == n and sc["rows"][0].shape == (S, 7, K)
    g, gu = restated_gradients(K, S, rows_of, panels)
    stage, ustage = stages(K, S, rows_of)
    only = set(range(min(n, 8)))
    more = only | ({36, 37, 38, 39, 64} if n == 65 else set())           # one more of each class (j % 4: fast or slow, ragged or not), and the row past the block
    seen = set()
    for union, who in ((False, "i"), (True, "i"), (True, "j"), (True, "both")):
        what = f"K {K} S {S} n {n} panels {panels} {'all pairs' if union else 'catalogue'} who {who}"
        side, cols, grads, stg = (sc["urows"], None, gu, ustage) if union else (sc["rows"], sc["cat"], g, stage)
        sens, Es, status = AW.window_sensitivity(grads, side, stg, who, cols)
        res = run(sc, "sens", union, who, panels=panels, return_state_gradient=True)
        assert np.array_equal(res.status, status), (what, res.status, status)
        wout, wstatus = window_bits(sc, union, panels)
        mine = np.column_stack([res.p, res.start, res.entries, res.rate_max, res.t_rate_max, res.window])
        assert mine.tobytes() == wout.tobytes() and np.array_equal(res.status, wstatus), (what, np.argwhere(~((mine == wout) | np.isnan(wout)))[:10])
        ok = status == 0
        assert ok.any() and np.isnan(res.sens[~ok]).all() and np.isfinite(res.sens[ok]).all()
        ratio = np.abs(res.sens[ok] - sens[ok]) / np.where(Es[ok] > 0.0, Es[ok], 1.0)
        moved = [sl for sl in range(sens.shape[1]) if (who, sl) in (("i", 0), ("j", 1), ("both", 0), ("both", 1))]
        assert (np.abs(res.sens[ok] - sens[ok]) <= Es[ok]).all(), (what, float(ratio.max()))
        assert all(np.abs(res.sens[ok][:, sl]).max() > 0.0 for sl in moved) and not any(res.sens[ok][:, sl].any() for sl in range(sens.shape[1]) if sl not in moved)
        worst_c = 0.0
        for r, e in enumerate(grads):
            if ok[r] and e["R"] > 0.0:
                assert (np.abs(res.state_grad[r] - e["c"]) <= e["Ec"]).all(), (what, r)
                worst_c = max(worst_c, float((np.abs(res.state_grad[r] - e["c"]) / np.where(e["Ec"] > 0.0, e["Ec"], 1.0)).max()))
        rs = sorted(only if union else more)
        out, du, st2, (Eo, Ed) = AW.avoidance_window(grads, sens, Es, status, side, stg, TARGET, TOL, MAX_EVAL, panels, who, cols, only=set(rs))
        av = run(sc, "avoid", union, who, panels=panels, return_sensitivities=True)
        assert av.sens.tobytes() == res.sens.tobytes(), what
        still = [sl for sl in range(sens.shape[1]) if sl not in moved]
        fine = av.status == 0
        assert not av.du[fine][:, still].any() and not av.dv[fine][:, [sl for sl in (0, 1) if sl not in moved]].any()
        assert not av.umax[fine][:, [sl for sl in (0, 1) if sl not in moved]].any()
        went = fine & (av.alpha > 0.0)                                   # (none at K = 2 with who = j: the window is cut at the object's first node)
        assert all((av.dv[went][:, sl] > 0.0).all() and av.du[went][:, sl].any(axis=(1, 2)).all() for sl in moved)
        assert np.array_equal(av.status[rs], st2[rs]), (what, av.status[rs], st2[rs])
        seen |= set(av.status.tolist())
        good = [r for r in rs if st2[r] == 0]
        assert np.isnan(av.out[av.status != 0]).all() and np.isnan(av.du[av.status != 0]).all()
        for r in good:
            fin = np.isfinite(Eo[r])
            assert (np.abs(av.out[r] - out[r])[fin] <= Eo[r][fin]).all(), (what, r, av.out[r], out[r], Eo[r])
            assert (np.abs(av.du[r] - du[r]) <= Ed[r]).all(), (what, r)
        done = (av.status == 0) & (av.alpha > 0.0)
        assert (np.abs(np.log(av.p1[done] / TARGET)) <= TOL).all() and (av.evals[done] >= 1).all() and (av.evals[done] <= MAX_EVAL).all()
        at_rest = (av.status == 0) & (av.alpha == 0.0)
        assert (av.p0[at_rest] <= TARGET).all() and not av.du[at_rest].any() and (av.p0[done] > TARGET).all()
        print(f"{what}: manoeuvre statuses {np.bincount(av.status, minlength=10).tolist()}, evaluations up to {int(np.nan_to_num(av.evals).max())}")
        print(f"{what}: worst |device - restated| / bound: sens {float(ratio.max()):.3e}, state gradient {worst_c:.3e}")
    if n == 65:
        assert {0, AW.ST_SINGULAR} <= seen                               # rows that manoeuvre, and the same object twice


def av_bits(r):
    return r.out.tobytes(), r.du.tobytes(), r.status.tobytes()


def test_same_bits():
    """with and without sens / state_grad; one row alone against the same row inside the list; a second context of the same device
    against the first; devices=[0, 0] against one device"""
    from mpconstellation_amd import conjunction as cj, _ffi
    sc = scene(30)
    a = run(sc, "sens", panels=3, return_state_gradient=True)
    b = run(sc, "sens", panels=3)
    c = run(sc, "sens", panels=3, devices=[0, 0], return_state_gradient=True)
    assert b.state_grad is None and sens_bits(a) == sens_bits(b) == sens_bits(c) and a.state_grad.tobytes() == c.state_grad.tobytes()
    m = run(sc, "avoid", panels=3, return_sensitivities=True)
    m2 = run(sc, "avoid", panels=3)
    m3 = run(sc, "avoid", panels=3, devices=[0, 0], return_sensitivities=True)
    assert m2.sens is None and av_bits(m) == av_bits(m2) == av_bits(m3) and m.sens.tobytes() == m3.sens.tobytes() == a.sens.tobytes()
    assert (m.status == 0).sum() >= 10 and (m.alpha[m.status == 0] > 0.0).any()
    for r in (6, 64):
        one = run(sc, "avoid", panels=3, pairs=sc["pairs"][r:r + 1], half=sc["half"][r:r + 1], return_sensitivities=True)
        assert one.out.tobytes() == m.out[r:r + 1].tobytes() and one.du.tobytes() == m.du[r:r + 1].tobytes() and one.sens.tobytes() == m.sens[r:r + 1].tobytes()
        s1 = run(sc, "sens", panels=3, pairs=sc["pairs"][r:r + 1], half=sc["half"][r:r + 1], return_state_gradient=True)
        assert s1.sens.tobytes() == a.sens[r:r + 1].tobytes() and s1.state_grad.tobytes() == a.state_grad[r:r + 1].tobytes()
    # the second context of device 0, by the block call the wrappers make
    Y, units, span, P, radius, ns = sc["rows"]
    n, K = len(sc["pairs"]), Y.shape[2]
    out = dict(out=np.empty((n, _ffi.NAW)), du=np.empty((n, 1, 3, K)), sens=None, status=np.zeros(n, dtype=np.int32))
    cols = cj._check_side(*sc["cat"][:5], sc["cat"][5], "cat_")
    cj._avoidance_window_call(sc["pairs"], sc["half"], device=0, slot=1, out=out, rows=sc["rows"] + (sc["U"], sc["consts"]), cols=cols,
                              mu=C.MU_EARTH, panels=3, who=0, flags=0, max_step=cj.DEFAULT_MAX_STEP, atmosphere=None, target_p=TARGET, tol=TOL,
                              max_eval=MAX_EVAL)
    assert (out["out"].tobytes(), out["du"].tobytes(), out["status"].tobytes()) == av_bits(m)


def test_statuses_in_one_call():
    """a bad index, t outside a span, the same object twice (|d| = 0), R <= 0, a half window that is not finite and a mover whose
    linearisation fails (a mass of zero: MPCX_ST_MASS; with an indefinite covariance as well, the window rule's MPCX_ST_NUMERIC comes
    first, as in the restatement), each between good rows: failed rows NaN, R <= 0 zeros with status 0, the same
    object twice zero sensitivities with status 0 and MPCX_ST_SINGULAR from the manoeuvre, the good rows the bytes of a call without
    the others"""
    from mpconstellation_amd import conjunction as cj
    sc = scene(30)
    (Y, units, span, P, radius, ns), U, consts = sc["urows"], sc["uU"], sc["uconsts"]
    S = 5
    Y, radius = Y.copy(), radius.copy()
    slow = [j for j in range(65) if j % 4 >= 2 and j != 3]
    last = [j for j in slow if sc["pairs"][j, 0] != sc["pairs"][3, 0]][-1]
    dead = int(sc["pairs"][last, 0])                                     # the satellite that cannot be linearised, and a row of its own
    good = [j for j in slow if sc["pairs"][j, 0] != dead][:5]
    pick = [good[0], good[1], good[1], good[2], 3, good[3], good[4], good[4], good[0], last, good[1]]
    rows, half = sc["upairs"][pick].copy(), sc["half"][pick].copy()
    P = P.copy()
    P[int(rows[10, 1])] = -100.0 * P[int(rows[10, 1])]                   # row 10 fails both ways: an indefinite covariance (the window
    rows[10, 0] = dead                                                   # rule's MPCX_ST_NUMERIC, which comes first) and the dead mover
    rows[1, 1] = len(Y)                                                  # no such object
    rows[2, 3] = 1.0e6                                                   # outside both spans
    j5 = int(rows[5, 1])
    radius[j5] = -radius[int(rows[5, 0])]                                # R = 0 exactly
    half[7] = np.inf
    Y[dead, 6, :] = 0.0                                                  # a mover that cannot be linearised
    args = dict(radius=radius, Y=Y, U=U, units=units, span=span, consts=consts, P=P, ns=ns, panels=3)
    res = cj.collision_window_sensitivity(rows, half_window=half, return_state_gradient=True, **args)
    av = cj.avoidance_window(rows, TARGET, tol=TOL, max_eval=MAX_EVAL, half_window=half, return_sensitivities=True, **args)
    B = AW.ST_BADK
    print("statuses", res.status, av.status)
    assert res.status.tolist() == [0, B, B, 0, 0, 0, 0, B, 0, 1, AW.ST_NUMERIC]
    assert av.status.tolist()[:4] == [0, B, B, 0] and av.status[4] == AW.ST_SINGULAR and av.status.tolist()[5:] == [0, 0, B, 0, 1, AW.ST_NUMERIC]
    for r in (1, 2, 7, 9, 10):
        assert np.isnan(res.sens[r]).all() and np.isnan(res.state_grad[r]).all() and np.isnan(res.p[r]) and np.isnan(av.out[r]).all() and np.isnan(av.du[r]).all()
    assert res.p[4] > TARGET and not res.sens[4].any() and not res.state_grad[4].any() and np.isnan(av.out[4]).all() and np.isnan(av.du[4]).all()
    assert (res.p[5], res.start[5], res.entries[5]) == (0.0, 0.0, 0.0) and not res.sens[5].any() and not res.state_grad[5].any()
    assert not av.out[5].any() and not av.du[5].any()
    keep = [0, 3, 6, 8]
    assert np.isfinite(res.sens[keep]).all() and res.sens[keep][:, 0].any(axis=(1, 2)).all() and av.sens.tobytes() == res.sens.tobytes()
    # the restatement's statuses (it needs no stage records for rows that fail; the good rows get the device's)
    side = (Y, units, span, P, radius, ns)
    grads = AW.row_gradients(rows, side, half, 3)
    dstat = np.zeros(len(Y), dtype=np.int32); dstat[dead] = 1
    Yf = np.nan_to_num(Y, nan=1.0); Yf[dead, 6, :] = 1.0
    _, _, ref_status = AW.window_sensitivity(grads, side, device_stage(Yf, U, units, span, consts, ns), "i", None, disc_status=dstat)
    assert np.array_equal(res.status, ref_status), (res.status, ref_status)
    alone = cj.collision_window_sensitivity(rows[keep], half_window=half[keep], return_state_gradient=True, **args)
    alone_av = cj.avoidance_window(rows[keep], TARGET, tol=TOL, max_eval=MAX_EVAL, half_window=half[keep], **args)
    assert alone.sens.tobytes() == res.sens[keep].tobytes() and alone.state_grad.tobytes() == res.state_grad[keep].tobytes()
    assert alone.p.tobytes() == np.ascontiguousarray(res.p[keep]).tobytes()
    assert alone_av.out.tobytes() == av.out[keep].tobytes() and alone_av.du.tobytes() == av.du[keep].tobytes()


def test_c_abi_refuses_bad_arguments():
    from mpconstellation_amd import _ffi
    lib, ctx = _ffi.load(), _ffi.context(0)
    S, K, n = 2, 5, 3
    Y, U, units, span, consts = np.ones((S, 7, K)), np.zeros((S, 3, K)), np.ones((S, 2)), np.array([[0.0, 1.0]] * S), np.ones((S, 8))
    P, radius, pairs, half = np.zeros((S, K, 6, 6)), np.ones(S), np.zeros((n, 4)), np.ones(n)
    out, wout, du, sens, st = np.zeros((n, _ffi.NAW)), np.zeros((n, _ffi.NPW)), np.zeros((n, 2, 3, K)), np.zeros((n, 2, 3, K)), np.zeros(n, dtype=np.int32)
    d, i = _ffi.dptr, _ffi.iptr
    none = (0, 0, None, None, None, None, None, None)
    cat = (S, K, None, d(Y), d(units), d(span), d(P), d(radius))

    def aw(n=n, S=S, K=K, flags=0, max_step=1e-2, P=d(P), radius=d(radius), cols=none, mu=C.MU_EARTH, half=d(half), panels=2, who=0, target=1e-4,
           tol=1e-6, max_eval=10, out=d(out), du=d(du), st=i(st)):
        return lib.mpcx_avoidance_window(ctx, n, d(pairs), S, K, None, d(Y), d(U), d(units), d(span), d(consts), flags, max_step, P, radius, *cols, mu,
                                         half, panels, who, target, tol, max_eval, out, du, None, st)

    def cs(n=n, S=S, K=K, flags=0, max_step=1e-2, P=d(P), radius=d(radius), cols=none, mu=C.MU_EARTH, half=d(half), panels=2, who=0, out=d(wout),
           sens=d(sens), st=i(st)):
        return lib.mpcx_collision_window_sensitivity(ctx, n, d(pairs), S, K, None, d(Y), d(U), d(units), d(span), d(consts), flags, max_step, P, radius,
                                                     *cols, mu, half, panels, who, out, sens, None, st)
    shared = (dict(n=0), dict(S=0), dict(K=1), dict(mu=0.0), dict(who=3), dict(who=-1), dict(flags=4), dict(flags=_ffi.FLAG_ATMO), dict(max_step=0.0),
              dict(cols=cat, who=1), dict(cols=cat, who=2), dict(cols=cat[:6] + (None, d(radius))), dict(cols=cat[:7] + (None,)),
              dict(cols=(0, K) + cat[2:]), dict(cols=(S, 1) + cat[2:]), dict(P=None), dict(radius=None), dict(half=None), dict(panels=0),
              dict(panels=_ffi.PW_MAX_PANELS + 1), dict(out=None), dict(st=None))
    for bad in shared + (dict(target=0.0), dict(target=1.0), dict(target=-0.5), dict(target=np.nan), dict(tol=0.0), dict(tol=np.inf), dict(tol=np.nan),
                         dict(max_eval=0), dict(du=None)):
        out[:] = 7.0
        assert aw(**bad) == -2, bad
        assert (b"avoidance_window" in lib.mpcx_last_error(ctx) or b"ATMO" in lib.mpcx_last_error(ctx)) and (out == 7.0).all()
    for bad in shared + (dict(sens=None),):
        wout[:] = 7.0
        assert cs(**bad) == -2, bad
        assert (b"collision_window_sensitivity" in lib.mpcx_last_error(ctx) or b"ATMO" in lib.mpcx_last_error(ctx)) and (wout == 7.0).all()
    for w in (lib.mpcx_avoidance_window_workspace_bytes, lib.mpcx_collision_window_sensitivity_workspace_bytes):
        assert w(0, 2, 5, 1) == 0 and w(3, 0, 5, 1) == 0 and w(3, 2, 1, 1) == 0 and w(3, 2, 5, 0) == 0 and w(3, 2, 5, 65) == 0
        assert w(3, 2, 5, 4) >= 2 * 4 * _ffi.STAGE_DOUBLES * 8 + 3 * 2 * 5 * 6 * 8
    assert aw() == 0 and cs() == 0 and (st == C.ST_NUMERIC).all() and np.isnan(out).all()    # (all zeros: no covariance to factor)


# |ln(P_flown / target_p)| of the end-to-end test, measured on the device when this file was written (profiles/avoidance_window.txt)
FLOWN_MEASURED = 1.365e-1


def test_end_to_end_planted_slow_pair():
    """The host tests' slow pair (test_avoidance_window_host.pair_on_arc: 120 m, a few m/s) on the arc the device flies:
    avoidance_window to a target two decades below P0 -> apply -> propagate_batch -> screen_track finds the event again ->
    collision_probability_window with P as given.  The flown probability must be below P0; its distance from the target in ln is the
    linearisation's (the dynamics are linear in the manoeuvre only to first order, and the event has moved in time), which nothing
    here removes.  Measured when written: P0 2.856e-3, target 2.856e-5, predicted 2.856083e-5 after 9 evaluations; flown, the event
    is 48.55 s earlier at 1114.8 m and P = 3.274e-5: |ln(P_flown / target_p)| = 0.1365 (FLOWN_MEASURED).  Asserted at twice that."""
    from mpconstellation_amd import conjunction as cj
    from test_avoidance_gpu import arc_on_device
    from test_avoidance_window_host import pair_on_arc, HALF
    a = AR.arc_setup()
    x = arc_on_device(a["U"])
    t, rows, cat, pairs = pair_on_arc(x, a, 20.37)
    Y, units, span, P, radius, _ = rows
    consts, U = a["consts"][None], a["U"][None]
    win0 = cj.collision_probability_window(pairs, radius, Y, units, span, P, HALF, panels=2, cat=cat)
    target = 1e-2 * win0.p[0]
    av = cj.avoidance_window(pairs, target, radius, Y, U, units, span, consts, P, HALF, panels=2, cat=cat)
    assert win0.status.tolist() == [0] and av.status.tolist() == [0] and av.p0[0] == win0.start[0] + win0.entries[0]
    assert abs(np.log(av.p1[0] / target)) <= cj._ffi.AW_DEFAULT_TOL
    U2 = av.apply(U, 0)
    x2 = arc_on_device(U2[0])
    found, info, st, _, _ = cj.screen_track(pairs, float(span[0, 0]), float(span[0, 1]), Y=x2[None], units=units, span=span, cat_Y=cat[0], cat_units=cat[1],
                                            cat_span=cat[2], M=4 * (AR.SCENE["K"] - 1) + 1)
    assert st.tolist() == [0] and np.isfinite(found[0, 3])
    win1 = cj.collision_probability_window(found, radius, x2[None], units, span, P, HALF, panels=2, cat=cat)
    gap = abs(np.log(win1.p[0] / target))
    print(f"P0 {win0.p[0]:.4e}, target {target:.4e}, predicted {av.p1[0]:.6e} after {int(av.evals[0])} evaluations, dv {av.dv[0, 0]:.4f} m/s, umax "
          f"{av.umax[0, 0]:.3e}; flown: event at {found[0, 3] - t:+.2f} s, {found[0, 2]:.1f} m, P {win1.p[0]:.4e}, |ln(P_flown / target)| {gap:.4e} "
          f"(measured when written {FLOWN_MEASURED:.4e})")
    assert win1.status.tolist() == [0] and win1.p[0] < win0.p[0]
    assert gap <= 2.0 * FLOWN_MEASURED


def test_constellation_mpc_avoidance_window():
    """test_collision_window_gpu.py's three-satellite plan with satellite 0 moved to pass 500 m from satellite 1: the method returns
    the screen, the window probabilities and the manoeuvre of the module-level calls on the plan, bit for bit, and a du of the plan's
    shape"""
    from mpconstellation_amd import Satellite, ConstellationMPC, conjunction as cj
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
    scr, win, av = mpc.avoidance_window(1000.0, P0, 5.0, 60.0, 1e-9, panels=2, q=1e-8, who="both")
    print("planted pair:", scr.pairs, "window p", win.p, "manoeuvre", av.out, "status", av.status)
    assert scr.pairs[:, :2].tolist() == [[0, 1]] and win.status.tolist() == [0] and av.status.tolist() == [0]
    assert av.du.shape == (1, 2, 3, X.shape[2]) and av.p0[0] == win.start[0] + win.entries[0] and av.p0[0] > 1e-9
    assert abs(np.log(av.p1[0] / 1e-9)) <= cj._ffi.AW_DEFAULT_TOL and av.du[0, 0].any() and av.du[0, 1].any()
    assert av.apply(mpc._plan[1], 0).shape == mpc._plan[1].shape
    P = cj.covariance(X, w["units"], w["span"], mpc.consts, P0, U=mpc._plan[1], ns=w["ns"], q=1e-8)
    av2 = cj.avoidance_window(scr, 1e-9, 5.0, X, mpc._plan[1], w["units"], w["span"], mpc.consts, P, 60.0, panels=2, ns=w["ns"], who="both")
    assert av.out.tobytes() == av2.out.tobytes() and av.du.tobytes() == av2.du.tobytes()
