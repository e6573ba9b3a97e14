"""numpy restatement of the collision probability over a time window (include/mpcx.h: mpcx_collision_probability_window) -- the same
formulas in the same order as csrc/collision_window.hip and the cw_* functions of csrc/collision_window_device.hpp, one array entry per
time node where the device has one lane -- an inner function on (R, d, w, A, B, D) that the host tests hold to independent truths,
and the full path from trajectories and node covariances.  Test infrastructure: the product never imports it."""
import functools

import numpy as np

import collision_reference as C

MU_EARTH = C.MU_EARTH
ST_OK, ST_NUMERIC, ST_BADK = C.ST_OK, C.ST_NUMERIC, C.ST_BADK
NPW = 7
PW_P, PW_START, PW_ENTRIES, PW_RATE_MAX, PW_T_RATE_MAX, PW_TA, PW_TB = range(NPW)
MAX_PANELS = 64
GL_X, GL_W = C.GL_X, C.GL_W
GL8_X, GL8_W = np.polynomial.legendre.leggauss(8)
NAZ, NMU = 32, 16
AZ_C = np.cos((np.arange(NAZ) + 0.5) * (2.0 * np.pi / NAZ))
AZ_S = np.sin((np.arange(NAZ) + 0.5) * (2.0 * np.pi / NAZ))
AZ_W = 0.09817477042468103                  # pi / 32: half a cos-theta interval's weight times 2 pi / 32
INV_SQRT_2PI, INV_SQRT2 = 0.3989422804014327, 0.7071067811865476
INV_2PI_32 = 0.06349363593424097            # (2 pi)^-3/2


def butterfly_sum(f):
    """the device's xor butterfly over 64 lanes (axis 0): pairwise 32, 16, ... apart"""
    n = 64
    while n > 1:
        n //= 2
        f = f[:n] + f[n:2 * n]
    return f[0]


# ---------------------------------------------------------------- the restatement: one time node per entry of the last axis
def sphere_frame(w):
    """w (3, T) -> wn (T,), the pole ew along w (the x axis where |w| is not positive), e1 from the coordinate axis on which |ew| is
    smallest (the first of equal ones) made orthogonal to ew, e2 = ew x e1: each (3, T)"""
    wn = np.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    pos = wn > 0.0
    with np.errstate(all="ignore"):
        ew = np.where(pos, w / wn, np.array([1.0, 0.0, 0.0])[:, None])
    ax = np.zeros(w.shape[1], dtype=int)
    ea = ew[0].copy()
    for c in (1, 2):
        less = np.abs(ew[c]) < np.abs(ea)
        ax = np.where(less, c, ax); ea = np.where(less, ew[c], ea)
    e1 = (np.arange(3)[:, None] == ax[None, :]) * 1.0 - ea * ew
    en = np.sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2])
    e1 = e1 / en
    e2 = np.array([ew[1] * e1[2] - ew[2] * e1[1], ew[2] * e1[0] - ew[0] * e1[2], ew[0] * e1[1] - ew[1] * e1[0]])
    return wn, ew, e1, e2


def node_setup(A, B, D):
    """A, B, D (3, 3, T): the relative state's covariance [[A, B^T], [B, D]] at every node -> ok (T,), Li (the inverse of A's
    Cholesky factor: l00, l10, l11, l20, l21, l22), W = B L^-T (3, 3, T), Sc = D - W W^T (c00, c01, c02, c11, c12, c22), cden =
    (2 pi)^-3/2 / sqrt(det A)"""
    with np.errstate(all="ignore"):
        ok = (A[0, 0] > 0.0) & np.isfinite(A[0, 0])
        l00 = np.sqrt(A[0, 0]); l10 = A[0, 1] / l00; l20 = A[0, 2] / l00
        r11 = A[1, 1] - l10 * l10
        ok &= (r11 > 0.0) & np.isfinite(r11)
        l11 = np.sqrt(r11); l21 = (A[1, 2] - l20 * l10) / l11
        r22 = A[2, 2] - l20 * l20 - l21 * l21
        ok &= (r22 > 0.0) & np.isfinite(r22)
        l22 = np.sqrt(r22)
        i00 = 1.0 / l00; i11 = 1.0 / l11; i22 = 1.0 / l22
        i10 = -(l10 * i00) * i11
        i21 = -(l21 * i11) * i22
        i20 = -(l20 * i00 + l21 * i10) * i22
        Li = (i00, i10, i11, i20, i21, i22)
        W = np.empty_like(B)
        for a in range(3):
            W[a, 0] = B[a, 0] * i00
            W[a, 1] = B[a, 0] * i10 + B[a, 1] * i11
            W[a, 2] = B[a, 0] * i20 + B[a, 1] * i21 + B[a, 2] * i22
        Sc = [D[a, b] - (W[a, 0] * W[b, 0] + W[a, 1] * W[b, 1] + W[a, 2] * W[b, 2]) for a in range(3) for b in range(a, 3)]
        cden = INV_2PI_32 * ((i00 * i11) * i22)
    return ok, Li, W, Sc, cden


def sphere_points(j, ew, e1, e2):
    """The points (j, k) of the sphere rule for the cos theta nodes j (an index array; node j of 16: the 8 Gauss-Legendre nodes on
    [-1, 0], then the 8 on [0, 1]) and all 32 azimuths k: weights of shape j.shape + (1,) and the unit vectors n (3,) + j.shape +
    (32,) + the frame's trailing axes (ew, e1, e2 (3, ...)).  Elementwise the device's expressions; only the loops are array axes."""
    j = np.asarray(j)
    mu = 0.5 * (GL8_X[j & 7] + np.where(j < 8, -1.0, 1.0))
    st = np.sqrt((1.0 - mu) * (1.0 + mu))
    wq = (GL8_W[j & 7] * AZ_W)[..., None]
    tail = (1,) * (ew.ndim - 1)
    mu, st = mu.reshape(mu.shape + (1,) + tail), st.reshape(st.shape + (1,) + tail)
    ca, sa = AZ_C.reshape((NAZ,) + tail), AZ_S.reshape((NAZ,) + tail)
    lead = (3,) + (1,) * (j.ndim + 1)
    f = lambda v: v.reshape(lead + v.shape[1:])
    n = mu * f(ew) + st * (ca * f(e1) + sa * f(e2))
    return wq, n


def whitened(n, r, d, Li):
    i00, i10, i11, i20, i21, i22 = Li
    x0 = r * n[0] - d[0]; x1 = r * n[1] - d[1]; x2 = r * n[2] - d[2]
    z0 = i00 * x0; z1 = i10 * x0 + i11 * x1; z2 = i20 * x0 + i21 * x1 + i22 * x2
    return z0, z1, z2


def entry_rate(R, d, w, A, B, D):
    """The rate at which probability enters the sphere of radius R at every node: d, w (3, T) the mean of the relative position and
    velocity, [[A, B^T], [B, D]] (each (3, 3, T)) their covariance -> ok (T,), rate (T,).  512 sphere points, summed in order."""
    from scipy.special import erfc
    _, ew, e1, e2 = sphere_frame(w)
    ok, Li, W, Sc, cden = node_setup(A, B, D)
    with np.errstate(all="ignore"):
        wq, n = sphere_points(np.arange(NMU), ew, e1, e2)                # n (3, 16, 32, T)
        z0, z1, z2 = whitened(n, R, d, Li)
        dens = np.exp(-0.5 * (z0 * z0 + z1 * z1 + z2 * z2))
        v0 = (n[0] * (w[0] + (W[0, 0] * z0 + W[0, 1] * z1 + W[0, 2] * z2)) + n[1] * (w[1] + (W[1, 0] * z0 + W[1, 1] * z1 + W[1, 2] * z2))
              + n[2] * (w[2] + (W[2, 0] * z0 + W[2, 1] * z1 + W[2, 2] * z2)))
        s2 = (n[0] * (Sc[0] * n[0] + Sc[1] * n[1] + Sc[2] * n[2]) + n[1] * (Sc[1] * n[0] + Sc[3] * n[1] + Sc[4] * n[2])
              + n[2] * (Sc[2] * n[0] + Sc[4] * n[1] + Sc[5] * n[2]))
        s = np.sqrt(np.where(s2 > 0.0, s2, 1.0))
        a = v0 / s
        E = np.where(s2 > 0.0, s * (np.exp(-0.5 * a * a) * INV_SQRT_2PI) - v0 * (0.5 * erfc(a * INV_SQRT2)), np.maximum(-v0, 0.0))
        term = wq[..., None] * (dens * E)
        acc = np.zeros(d.shape[1])
        for j in range(NMU):
            for k in range(NAZ):
                acc = acc + term[j, k]
        rate = ((R * R) * cden) * acc
    return ok, rate


def ball_probability(R, d, w, A):
    """P(|rho| <= R) for rho ~ N(d, A) (d, w (3,), A (3, 3); w only places the sphere rule's pole): 8 Gauss-Legendre radii times the
    sphere rule, dealt over 64 lanes -- lane l has radius l / 8 and the cos theta nodes 2 (l % 8), 2 (l % 8) + 1 -- and summed by the
    butterfly -> ok, probability"""
    _, ew, e1, e2 = sphere_frame(w[:, None])
    A3 = A[:, :, None]
    ok, Li, _, _, cden = node_setup(A3, np.zeros_like(A3), np.zeros_like(A3))
    lane = np.arange(64)
    i, j0 = lane >> 3, 2 * (lane & 7)
    with np.errstate(all="ignore"):
        r = R * (0.5 + 0.5 * GL8_X[i])
        wr = ((0.5 * R) * GL8_W[i]) * (r * r)
        wq, n = sphere_points(np.stack([j0, j0 + 1], axis=1), ew[:, 0], e1[:, 0], e2[:, 0])      # n (3, 64, 2, 32)
        z0, z1, z2 = whitened(n, r[:, None, None], d, [x[0] for x in Li])
        term = wq * np.exp(-0.5 * (z0 * z0 + z1 * z1 + z2 * z2))
        acc = np.zeros(64)
        for j in range(2):
            for k in range(NAZ):
                acc = acc + term[:, j, k]
        return bool(ok[0]), float(cden[0] * butterfly_sum(wr * acc))


def window_probability(R, ta, tb, panels, state, diagnostics=None):
    """state(tau (T,)) -> (d, w, A, B, D) at the times tau: the window [ta, tb] in `panels` equal panels of 64 Gauss-Legendre nodes,
    the ball term at ta -> (status, [p, start, entries, rate_max, t_rate_max, ta, tb]).  diagnostics: a dict that receives what
    rounding_bound needs of the row's time nodes."""
    nan = np.full(NPW, np.nan)
    if not np.isfinite(R):
        return ST_NUMERIC, nan
    if not R > 0.0:
        return ST_OK, np.array([0.0, 0.0, 0.0, 0.0, ta, ta, tb])
    hp = (tb - ta) / panels
    entries, rmax, tmax, good = 0.0, -np.inf, ta, True
    for p in range(panels):
        tau = (ta + p * hp) + (0.5 * hp) * (1.0 + GL_X)
        d, w, A, B, D = state(tau)
        ok, rate = entry_rate(R, d, w, A, B, D)
        good = good and bool(ok.all())
        if diagnostics is not None and good:
            _diagnose(diagnostics, d, A)
        entries = entries + butterfly_sum(((0.5 * hp) * GL_W) * rate)
        seen = ~np.isnan(rate)                                           # (the device's fmax passes a NaN by)
        if seen.any() and rate[seen].max() > rmax:
            rmax = rate[seen].max(); tmax = tau[seen][int(np.argmax(rate[seen]))]
    d, w, A, _, _ = state(np.array([ta]))
    ok, start = ball_probability(R, d[:, 0], w[:, 0], A[:, :, 0])
    total = start + entries
    if not (good and ok) or not np.isfinite(total):
        return ST_NUMERIC, nan
    return ST_OK, np.array([min(total, 1.0), start, entries, rmax, tmax, ta, tb])


def _diagnose(dg, d, A):
    """over the time nodes seen so far: the largest cond(A), the smallest sigma (sqrt of A's smallest eigenvalue), the smallest
    Mahalanobis distance of the mean from the origin"""
    lam = np.linalg.eigvalsh(np.transpose(A, (2, 0, 1)))
    mah = np.sqrt(np.einsum("at,tab,bt->t", d, np.linalg.inv(np.transpose(A, (2, 0, 1))), d))
    dg["cond"] = max(dg.get("cond", 0.0), float((lam[:, 2] / lam[:, 0]).max()))
    dg["sigma_min"] = min(dg.get("sigma_min", np.inf), float(np.sqrt(lam[:, 0].min())))
    dg["mahal"] = min(dg.get("mahal", np.inf), float(mah.min()))


def rounding_bound(R, dg):
    """The relative difference two correct fp64 evaluations of one row may show (fused or unfused multiply-adds, other exp / erfc),
    from the arithmetic.  Positions of 7e6 m through the Hermite's few operations differ by about 2e-7 m (test_conjunction_gpu.py),
    which moves d by as much and the density by its logarithmic slope m / sigma_min, m the Mahalanobis distance of the sphere points
    that still count: the closest approach's plus R / sigma_min plus 3 (three sigma further out the weight has fallen by e^-4.5).
    The exponent |z|^2 / 2 = x^T A^-1 x / 2 <= m^2 / 2 is formed through the Cholesky factor of a matrix that is itself two six-term
    products: its rounding is gamma cond(A) m^2 with gamma = 64 eps; the sums' and special functions' own 1e-11 (1 + m^2) as in
    test_collision_gpu.py."""
    m = dg["mahal"] + R / dg["sigma_min"] + 3.0
    return 2e-7 * m / dg["sigma_min"] + (64.0 * np.finfo(np.float64).eps * dg["cond"] + 1e-11) * (1.0 + m * m)


# ---------------------------------------------------------------- the restatement: objects on their own nodes
def _ordered(X, Y):
    """X @ Y for stacks (T, 6, 6), every sum run m = 0 .. 5 in order"""
    acc = X[:, :, 0:1] * Y[:, 0:1, :]
    for m in range(1, 6):
        acc = acc + X[:, :, m:m + 1] * Y[:, m:m + 1, :]
    return acc


def gradient(x, mu):
    """G = mu (3 x x^T - |x|^2 I) / |x|^5 at the positions x (3, T) -> (3, 3, T), short_arc_rows' expression"""
    r2 = x[0] * x[0] + x[1] * x[1] + x[2] * x[2]
    r1 = np.sqrt(r2); r5 = r2 * r2 * r1
    return np.array([[mu * (3.0 * x[a] * x[b] - (r2 if a == b else 0.0)) / r5 for b in range(3)] for a in range(3)])


def short_arc_transition(r, v, dt, mu):
    """The 6 x 6 short-arc transition (T, 6, 6) from the node positions r and velocities v (3, T) over the times dt (T,).  Position
    rows [I + G0 dt^2/2 | dt I + G0 dt^3/6] (collision_reference.short_arc_rows to the bit); velocity rows their derivative int_0^dt
    G(s) Phi_r(s) ds by Simpson's rule on the gradient at the node, the middle and the end of the arc (r + v s + a s^2 / 2):
    [(G0 + 4 Gm + Ge) dt/6 + G0^2 dt^3/6 | I + (2 Gm + Ge) dt^2/6]."""
    r2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2]
    r3 = r2 * np.sqrt(r2)
    ca = dt * dt / 2.0; cb = dt * dt * dt / 6.0; hd = 0.5 * dt; ch = hd * hd / 2.0
    ac = -mu * r / r3
    rm = r + v * hd + ac * ch
    re = r + v * dt + ac * ca
    G0, Gm, Ge = gradient(r, mu), gradient(rm, mu), gradient(re, mu)
    c6 = dt / 6.0; d6 = dt * dt / 6.0
    F = np.empty((len(dt), 6, 6))
    for a in range(3):
        for b in range(3):
            G = G0[a, b]
            Q = G0[a, 0] * G0[0, b] + G0[a, 1] * G0[1, b] + G0[a, 2] * G0[2, b]
            F[:, a, b] = (1.0 if a == b else 0.0) + G * ca
            F[:, a, 3 + b] = (dt if a == b else 0.0) + G * cb
            F[:, 3 + a, b] = (G + 4.0 * Gm[a, b] + Ge[a, b]) * c6 + Q * cb
            F[:, 3 + a, 3 + b] = (1.0 if a == b else 0.0) + (2.0 * Gm[a, b] + Ge[a, b]) * d6
    return F


def object_at(side, o, tau, mu):
    """object o of side = (Y, units, span, P, radius, ns) at the times tau (T,), all inside its span: position and velocity (3, T)
    from the cubic Hermite on its nodes (collision_reference.state_and_cov_at's lines), and the nearest node's 6 x 6 covariance
    carried over by the short-arc transition, upper triangle mirrored (T, 6, 6)"""
    Y, units, span, P, _, ns = side
    K = Y.shape[2]
    nn = K if ns is None else int(ns[o])
    ta, tb = span[o]
    hn = (tb - ta) / (nn - 1)
    u = (tau - ta) / hn
    k = np.clip(u.astype(int), 0, nn - 2)
    sg = u - k
    s2 = sg * sg; s3 = s2 * sg
    h00 = 2.0 * s3 - 3.0 * s2 + 1.0; h10 = s3 - 2.0 * s2 + sg; h01 = -2.0 * s3 + 3.0 * s2; h11 = s3 - s2
    g00 = 6.0 * s2 - 6.0 * sg; g10 = 3.0 * s2 - 4.0 * sg + 1.0; g01 = -6.0 * s2 + 6.0 * sg; g11 = 3.0 * s2 - 2.0 * sg
    L = units[o, 0]; V = L / units[o, 1]
    y = Y[o]
    p0 = y[0:3, k] * L; p1 = y[0:3, k + 1] * L
    m0 = hn * (y[3:6, k] * V); m1 = hn * (y[3:6, k + 1] * V)
    p = h00 * p0 + h10 * m0 + h01 * p1 + h11 * m1
    v = (g00 * p0 + g10 * m0 + g01 * p1 + g11 * m1) / hn
    kc = k + (sg >= 0.5)
    dt = tau - (ta + kc * hn)
    F = short_arc_transition(y[0:3, kc] * L, y[3:6, kc] * V, dt, mu)
    Cm = _ordered(_ordered(F, np.asarray(P[o, kc], dtype=np.float64)), np.transpose(F, (0, 2, 1)))
    iu = np.triu_indices(6)
    Cs = np.empty_like(Cm)
    Cs[:, iu[0], iu[1]] = Cm[:, iu[0], iu[1]]
    Cs[:, iu[1], iu[0]] = Cm[:, iu[0], iu[1]]
    return p, v, Cs


def relative_state(rows, cols, i, j, tau, mu):
    """(d, w, A, B, D) of the pair (i, j) at the times tau"""
    pa, va, Ca = object_at(rows, i, tau, mu)
    pb, vb, Cb = object_at(cols, j, tau, mu)
    Cs = np.transpose(Ca + Cb, (1, 2, 0))
    return pb - pa, vb - va, Cs[0:3, 0:3], Cs[3:6, 0:3], Cs[3:6, 3:6]


def _object_check(side, fidx, t):
    """cp_state's tests -> (status, object, span)"""
    Y, units, span, P, radius, ns = side
    N, _, K = Y.shape
    if not (fidx >= 0.0 and fidx < N):
        return ST_BADK, None, None
    o = int(fidx)
    nn = K if ns is None else int(ns[o])
    ta, tb = span[o]
    if nn < 2 or nn > K or not tb > ta or not (t >= ta and t <= tb):
        return ST_BADK, None, None
    return ST_OK, o, (ta, tb)


def collision_probability_window(pairs, rows, half_window, panels, cols=None, mu=MU_EARTH, bounds=None):
    """pairs (n, 4); rows, cols = (Y, units, span, P, radius, ns) (cols None: the columns are the rows); half_window a scalar or (n,)
    -> out (n, 7), status (n,).  bounds: an (n,) array that receives rounding_bound of every good row (NaN elsewhere)."""
    pairs = np.asarray(pairs, dtype=np.float64).reshape(-1, 4)
    cols = rows if cols is None else cols
    hw = np.broadcast_to(np.asarray(half_window, dtype=np.float64), (len(pairs),))
    out = np.full((len(pairs), NPW), np.nan)
    status = np.zeros(len(pairs), dtype=np.int32)
    for n, (i, j, _, t) in enumerate(pairs):
        h = hw[n]
        st, oa, sa = _object_check(rows, i, t)
        if st == ST_OK:
            st, ob, sb = _object_check(cols, j, t)
        if st == ST_OK and not (h > 0.0 and np.isfinite(h)):
            st = ST_BADK
        if st == ST_OK:
            ta = max(max(t - h, sa[0]), sb[0]); tb = min(min(t + h, sa[1]), sb[1])
            if not tb > ta:
                st = ST_BADK
        if st == ST_OK:
            R = float(rows[4][oa]) + float(cols[4][ob])
            dg = {}
            st, o = window_probability(R, ta, tb, panels, lambda tau: relative_state(rows, cols, oa, ob, tau, mu), dg)
            out[n] = o
            if bounds is not None:
                bounds[n] = rounding_bound(R, dg) if st == ST_OK and R > 0.0 else np.nan
        status[n] = st
    return out, status


# ---------------------------------------------------------------- shared scenes (computed once per size)
SCENE_KS, SCENE_PANELS, SCENE_N = (2, 3, 30), (1, 3), 65


@functools.lru_cache(maxsize=None)
def window_scene(K, seed=0):
    """Five satellites on random circular LEO orbits, K nodes 100 s apart, and a catalogue of 65 objects in rows of K nodes (every odd
    one with fewer in use -- K - 7, at least 2 -- and NaN behind them) on spans of their own.  Object j passes satellite i_j at t_j
    within 300 m: rows with j % 4 < 2 at a crossing angle of 0.5 .. 2.6 rad (km/s; half windows of 0.5 .. 1.5 s), the others along
    the satellite's own direction turned by at most 1e-4 rad (relative speed below 1 m/s; half windows of 60 .. 300 s, cut to the
    spans where K is small); object 3 IS satellite i_3 -- the same nodes, units and span: no relative position or speed at all.
    Random covariances at every node, radii of 1 .. 50 m.  -> rows, cat, pairs (65, 4), half (65,), and per panel count of
    SCENE_PANELS the restated out, status and rounding bound of the catalogue form.  Treat as read-only."""
    import conjunction_reference as R
    rng = np.random.default_rng(500 + 11 * K + seed)
    S, n = 5, SCENE_N
    orb = R.random_orbits(S, seed + 5)
    span_rows = (-1.0, 100.0 * (K - 1) + 1.0)
    T = span_rows[1] - span_rows[0]
    Y, units, span = R.trajectories(orb, K, span_rows)
    cY = np.full((n, 7, K), np.nan); cunits = np.empty((n, 2)); cspan = np.empty((n, 2)); cns = np.empty(n, dtype=np.int32)
    pairs = np.empty((n, 4)); half = np.empty(n)
    for j in range(n):
        i = int(rng.integers(S))
        t = float(rng.uniform(0.2 * T, 0.8 * T))
        p, v = R.kepler_state({k: x[i:i + 1] for k, x in orb.items()}, np.array([t]))
        p, v = p[0], v[0]
        e = rng.normal(size=3); e /= np.linalg.norm(e)
        miss = float(rng.uniform(0.0, 300.0))
        q = p + miss * e
        qh = q / np.linalg.norm(q)
        vh = v - (v @ qh) * qh; vh /= np.linalg.norm(vh)
        fast = j % 4 < 2
        ang = float(rng.uniform(0.5, 2.6)) if fast else float(rng.uniform(0.0, 1e-4))
        vhat = np.cos(ang) * vh + np.sin(ang) * np.cross(qh, vh)
        half[j] = float(rng.uniform(0.5, 1.5)) if fast else float(rng.uniform(60.0, 300.0))
        cns[j] = max(2, K - 7) if j % 2 else K
        cspan[j] = (span_rows[0] + float(rng.uniform(0.1, 0.1 * T)), span_rows[1] - float(rng.uniform(0.1, 0.1 * T)))
        if j == 3:
            cns[j], cspan[j], cY[j], cunits[j] = K, span[i], Y[i], units[i]
        else:
            cY[j, :, :cns[j]], cunits[j] = C.circular_through(q, vhat, t, int(cns[j]), cspan[j])
        pairs[j] = (i, j, miss, t)
    rows = (Y, units, span, C.random_covariances(rng, S, K), rng.uniform(1.0, 50.0, S), None)
    cat = (cY, cunits, cspan, C.random_covariances(rng, n, K), rng.uniform(1.0, 50.0, n), cns)
    ref = {}
    for panels in SCENE_PANELS:
        bounds = np.full(n, np.nan)
        out, status = collision_probability_window(pairs, rows, half, panels, cat, bounds=bounds)
        ref[panels] = (out, status, bounds)
    return dict(rows=rows, cat=cat, pairs=pairs, half=half, ref=ref)
