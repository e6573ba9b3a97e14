"""numpy restatement of mpcx_collision_probability_mc (include/mpcx.h, csrc/collision_mc.hip): the generator, the draws and the scan,
expression for expression where the order of operations matters.  The flight is not restated: the scan is fed trajectories."""
import numpy as np

ST_OK, ST_NUMERIC, ST_BADK = 0, 6, 9
EPS = np.finfo(np.float64).eps
_MASK = np.uint64(0xFFFFFFFF)
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
NMS = 5


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10: counter words (arrays broadcast against each other), key words (integers) -> four uint64 arrays of 32-bit words"""
    c = [np.asarray(x).astype(np.uint64) & _MASK for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(_M0), c[2] * np.uint64(_M1)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _MASK]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c


def uniform(a, b):
    """((a >> 5) 2^26 + (b >> 6) + 0.5) 2^-53 in the device's order; the tie at the top (all 53 bits set) is rounded down"""
    a, b = np.asarray(a).astype(np.uint64), np.asarray(b).astype(np.uint64)
    k = (a >> np.uint64(5)).astype(np.float64) * 67108864.0 + (b >> np.uint64(6)).astype(np.float64)
    return np.minimum((k + 0.5) * 2.0 ** -53, 1.0 - 2.0 ** -53)


def normals(sample, obj, block, side, seed):
    """the two normals of Philox block (sample, obj, block, side) under `seed` -> za, zb"""
    w = philox(sample, obj, block, side, seed & 0xFFFFFFFF, seed >> 32)
    u1, u2 = uniform(w[0], w[1]), uniform(w[2], w[3])
    rad = np.sqrt(-2.0 * np.log(u1))
    ang = 6.283185307179586 * u2
    return rad * np.cos(ang), rad * np.sin(ang)


def normal_bound(za, zb):
    """|device z - restated z| allowed: log and sincos of two libms differ by a few ulp -- the radius sqrt(-2 ln u) inherits half the
    logarithm's relative error, the angle 2 pi u carries one rounding of up to 2 pi eps / 2 into cos and sin, whose own error is an ulp
    of 1.  Summed generously: 16 eps (1 + radius) per normal."""
    return 16.0 * EPS * (1.0 + np.hypot(za, zb))


def factor(P0):
    """P0 = L L^T by columns with the header's zero-pivot rule (the upper triangle is read) -> (ok, L (6, 6) lower)"""
    P0 = np.asarray(P0, dtype=np.float64)
    L = np.zeros((6, 6))
    ok = True
    for j in range(6):
        tj = P0[j, j]
        if not (tj >= 0.0 and np.isfinite(tj)):
            ok = False
        d = tj
        for k in range(j):
            d = d - L[j, k] * L[j, k]
        tol = 1e-12 * tj
        reg = bool(d > tol)
        if not reg and not d >= -tol:
            ok = False
        L[j, j] = np.sqrt(d) if reg else 0.0
        for i in range(j + 1, 6):
            c = P0[j, i]
            for k in range(j):
                c = c - L[i, k] * L[j, k]
            if not reg and not c * c <= tol * P0[i, i]:
                ok = False
            L[i, j] = c / L[j, j] if reg else 0.0
    return ok, L


def state_normals(samples, obj, side, seed):
    """z (N, 6) of blocks 0..2 and the mass normal zm (N,) of block 3, with their bounds"""
    samples = np.asarray(samples)
    z, dz = np.empty((len(samples), 6)), np.empty((len(samples), 6))
    for b in range(3):
        za, zb = normals(samples, obj, b, side, seed)
        z[:, 2 * b], z[:, 2 * b + 1] = za, zb
        dz[:, 2 * b] = dz[:, 2 * b + 1] = normal_bound(za, zb)
    zm, zu = normals(samples, obj, 3, side, seed)
    return z, dz, zm, normal_bound(zm, zu)


def draw_initial(y_first, units, P0, m_var0, samples, obj, side, seed):
    """y0 (N, 7) of object `obj` in the listed samples and the bound (N, 7) on the device's difference from it: the normals' bounds
    pushed through L, eight roundings on every product sum, one on the final sum"""
    ok, L = factor(P0)
    z, dz, zm, dzm = state_normals(samples, obj, side, seed)
    D = np.array([units[0]] * 3 + [units[0] / units[1]] * 3)
    x = np.zeros((len(z), 6))
    for i in range(6):
        acc = L[i, 0] * z[:, 0]
        for j in range(1, i + 1):
            acc = acc + L[i, j] * z[:, j]
        x[:, i] = acc / D[i]
    sm = np.sqrt(m_var0)
    y0 = np.empty((len(z), 7))
    y0[:, :6] = y_first[None, :6] + x
    y0[:, 6] = y_first[6] + sm * zm
    bound = np.empty_like(y0)
    bound[:, :6] = (np.abs(L) @ dz.T).T / D + 8.0 * EPS * (np.abs(L) @ np.abs(z).T).T / D + EPS * np.abs(y0[:, :6])
    bound[:, 6] = sm * dzm + 4.0 * EPS * np.abs(sm * zm) + EPS * np.abs(y0[:, 6])
    return ok, y0, bound


def gates_frame(u):
    """u^ , e_1, e_2 of a thrust vector (3,) by the project's rule"""
    un = np.sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2])
    h = u / un
    ax, ea = 0, h[0]
    if abs(h[1]) < abs(ea):
        ax, ea = 1, h[1]
    if abs(h[2]) < abs(ea):
        ax, ea = 2, h[2]
    e1 = (np.arange(3) == ax).astype(np.float64) - ea * h
    e1 = e1 / np.sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2])
    e2 = np.array([h[1] * e1[2] - h[2] * e1[1], h[2] * e1[0] - h[0] * e1[2], h[0] * e1[1] - h[1] * e1[0]])
    return un, h, e1, e2


def draw_thrust(U, nn, execution, samples, obj, side, seed):
    """the executed thrust tables (N, 3, K) of object `obj` (U (3, K) or None, nn nodes in use, execution (5,) or None) and the bound on
    the device's difference: the three normals' bounds through s_par, s_perp, sixteen roundings on the frame and the sums"""
    samples = np.asarray(samples)
    K = U.shape[1] if U is not None else 0
    out = np.zeros((len(samples), 3, K))
    bound = np.zeros_like(out)
    if U is None:
        return out, bound
    for k in range(min(nn, K)):
        u = U[:, k].astype(np.float64)
        out[:, :, k] = u[None, :]
        if execution is None:
            continue
        fm, pm, fp, pp, off = execution
        un = np.sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2])
        if not un > off:
            continue
        un, h, e1, e2 = gates_frame(u)
        am, ap = pm * un, pp * un
        spar, sperp = np.sqrt(fm * fm + am * am), np.sqrt(fp * fp + ap * ap)
        z1, z2 = normals(samples, obj, 4 + 2 * k, side, seed)
        z3, zu = normals(samples, obj, 5 + 2 * k, side, seed)
        a1, a2, a3 = spar * z1, sperp * z2, sperp * z3
        for c in range(3):
            out[:, c, k] = u[c] + (a1 * h[c] + (a2 * e1[c] + a3 * e2[c]))
        d12, d3 = normal_bound(z1, z2), normal_bound(z3, zu)
        mag = np.abs(a1) + np.abs(a2) + np.abs(a3)
        bound[:, :, k] = (spar * d12 + sperp * (d12 + d3) + 16.0 * EPS * mag)[:, None] + EPS * np.abs(out[:, :, k])
    return out, bound


def gates_sigma(u, execution):
    """Sigma_k of mpcx_covariance_thrust_batch for one node"""
    fm, pm, fp, pp, off = execution
    un = np.linalg.norm(u)
    if not un > off:
        return np.zeros((3, 3))
    h = u / un
    return (fm * fm + (pm * un) ** 2) * np.outer(h, h) + (fp * fp + (pp * un) ** 2) * (np.eye(3) - np.outer(h, h))


# ---------------------------------------------------------------- the scan
def hermite_state(y, nn, span, units, t):
    """position (m) and velocity (m/s) at the times t (array) of the trajectory y (7, K) with nn nodes over span: cp_state's
    expressions -> p (len t, 3), v (len t, 3)"""
    t = np.asarray(t, dtype=np.float64)
    ta, tb = span
    L, Tu = units
    hn = (tb - ta) / float(nn - 1)
    u = (t - ta) / hn
    k = np.clip(u.astype(np.int64), 0, nn - 2)
    sg = u - k
    s2 = sg * sg
    s3 = s2 * sg
    h00, h10, h01, h11 = 2.0 * s3 - 3.0 * s2 + 1.0, s3 - 2.0 * s2 + sg, -2.0 * s3 + 3.0 * s2, s3 - s2
    g00, g10, g01, g11 = 6.0 * s2 - 6.0 * sg, 3.0 * s2 - 4.0 * sg + 1.0, -6.0 * s2 + 6.0 * sg, 3.0 * s2 - 2.0 * sg
    V = L / Tu
    p, v = np.empty((len(t), 3)), np.empty((len(t), 3))
    for c in range(3):
        p0, p1 = y[c, k] * L, y[c, k + 1] * L
        m0, m1 = hn * (y[3 + c, k] * V), hn * (y[3 + c, k + 1] * V)
        p[:, c] = h00 * p0 + h10 * m0 + h01 * p1 + h11 * m1
        v[:, c] = (g00 * p0 + g10 * m0 + g01 * p1 + g11 * m1) / hn
    return p, v


def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def interval_minimum(d0, d1, w0, w1, h, t0, t1):
    """mc_interval for arrays of intervals: q0, q1, qmin, tmin"""
    q0, q1 = _dot(d0, d0), _dot(d1, d1)
    qm, tm = q0.copy(), np.array(t0, dtype=np.float64).copy()
    later = q1 < qm
    qm[later], tm[later] = q1[later], t1[later]
    D = d1 - d0
    DD, b = _dot(D, D), _dot(d0, D)
    s = np.zeros_like(q0)
    good = (DD > 0.0) & np.isfinite(DD)
    with np.errstate(all="ignore"):
        s[good] = np.clip(-b[good] / DD[good], 0.0, 1.0)
    inner = (s > 0.0) & (s < 1.0)
    a0, a1 = h[:, None] * w0, h[:, None] * w1
    x = np.zeros_like(d0)
    for it in range(4):
        s2 = s * s
        s3 = s2 * s
        h00, h10, h01, h11 = 2.0 * s3 - 3.0 * s2 + 1.0, s3 - 2.0 * s2 + s, -2.0 * s3 + 3.0 * s2, s3 - s2
        x = h00[:, None] * d0 + h10[:, None] * a0 + h01[:, None] * d1 + h11[:, None] * a1
        if it == 3:
            break
        g00, g10, g01, g11 = 6.0 * s2 - 6.0 * s, 3.0 * s2 - 4.0 * s + 1.0, -6.0 * s2 + 6.0 * s, 3.0 * s2 - 2.0 * s
        k00, k10, k01, k11 = 12.0 * s - 6.0, 6.0 * s - 4.0, -12.0 * s + 6.0, 6.0 * s - 2.0
        x1 = g00[:, None] * d0 + g10[:, None] * a0 + g01[:, None] * d1 + g11[:, None] * a1
        x2 = k00[:, None] * d0 + k10[:, None] * a0 + k01[:, None] * d1 + k11[:, None] * a1
        g, gp = _dot(x, x1), _dot(x1, x1) + _dot(x, x2)
        step = inner & (gp > 0.0)
        with np.errstate(all="ignore"):
            s = np.where(step, np.clip(s - g / np.where(step, gp, 1.0), 0.0, 1.0), s)
    qs = _dot(x, x)
    better = inner & (qs < qm)
    qm[better], tm[better] = qs[better], (t0 + s * h)[better]
    return q0, q1, qm, tm


def scan_instants(ta, tb, scan):
    t = ta + np.arange(scan + 1, dtype=np.float64) * ((tb - ta) / float(scan))
    t[scan] = tb
    return t


def scan_relative(t, d, w, R):
    """the scan of one sample from the relative positions d and velocities w (scan + 1, 3) at the instants t -> (dmin, t_min,
    inside_start, entries) and the squared end distances (for a caller that wants to know how marginal the sample is)"""
    h = t[1:] - t[:-1]
    q0, q1, qm, tm = interval_minimum(d[:-1], d[1:], w[:-1], w[1:], h, t[:-1], t[1:])
    R2 = R * R
    entries = int(np.count_nonzero((q0 > R2) & ((q1 <= R2) | (qm <= R2))))
    best = qm.min()
    tbest = tm[qm == best].min()
    return (float(np.sqrt(best)), float(tbest), int(q0[0] <= R2), entries), np.concatenate([q0, q1[-1:]]), qm


def scan_pair(yi, ni, span_i, units_i, yj, nj, span_j, units_j, ta, tb, R, scan):
    """the scan of one sample from the two flown trajectories"""
    t = scan_instants(ta, tb, scan)
    pi, vi = hermite_state(yi, ni, span_i, units_i, t)
    pj, vj = hermite_state(yj, nj, span_j, units_j, t)
    return scan_relative(t, pj - pi, vj - vi, R)


def window(t, h, span_i, span_j):
    return max(t - h, span_i[0], span_j[0]), min(t + h, span_i[1], span_j[1])


def counts_of(samples):
    """counts (n, 6) from per-sample records (n, N, 5)"""
    st = samples[:, :, 4]
    ok = st == 0.0
    ins, ent = np.where(ok, samples[:, :, 2], 0.0).astype(np.int64), np.where(ok, samples[:, :, 3], 0.0).astype(np.int64)
    b = ins + ent
    return np.stack([np.full(len(samples), samples.shape[1], dtype=np.int64), (~ok).sum(1), ins.sum(1), ent.sum(1), (b * b).sum(1),
                     (ok & (b >= 1)).sum(1)], axis=1)


def out_of(counts, ta, tb):
    """out (n, 9) from the counts, the device's expressions"""
    counts = np.asarray(counts, dtype=np.int64)
    out = np.empty((len(counts), 9))
    for r, cn in enumerate(counts):
        N = float(cn[0] - cn[1])
        p, start, entries = cn[5] / N, cn[2] / N, cn[3] / N
        sb, sq = float(cn[2] + cn[3]), float(cn[4])
        dev = sq - sb * sb / N
        var = dev / (N - 1.0) if N > 1 and dev > 0.0 else 0.0
        out[r] = (p, np.sqrt(p * (1.0 - p) / N), start, entries, np.sqrt(var / N), (start + entries) - p, ta[r], tb[r], N)
    return out
