"""numpy restatement of the conjunction screen (include/mpcx.h: mpcx_ephemeris_batch, mpcx_conjunction_screen) -- the same formulas in
the same order as csrc/conjunction.hip, vectorised over satellites / pairs -- and an analytic generator of inclined circular Kepler
orbits (position and velocity at any t) to feed it and to know the truth.  Test infrastructure: the product never imports it."""
import functools

import numpy as np

MU_EARTH = 3.986004418e14
ST_BADK = 9


# ---------------------------------------------------------------- analytic orbits
def random_orbits(S, seed, r_lo=6.9e6, r_hi=7.3e6):
    """S inclined circular orbits: radius (m), inclination, node, phase at t = 0 -- a LEO shell, any geometry"""
    rng = np.random.default_rng(seed)
    return dict(R=rng.uniform(r_lo, r_hi, S), inc=rng.uniform(0.2, 1.7, S), raan=rng.uniform(0, 2 * np.pi, S), phase=rng.uniform(0, 2 * np.pi, S))


def orbit_rate(orb):
    return np.sqrt(MU_EARTH / orb["R"] ** 3)


def kepler_state(orb, t):
    """position (..., 3) in m and velocity (..., 3) in m/s of every orbit at its own time t (t broadcasts against the orbits)"""
    R, inc, raan = orb["R"], orb["inc"], orb["raan"]
    w = orbit_rate(orb)
    th = orb["phase"] + w * t
    u = np.stack([np.cos(raan), np.sin(raan), np.zeros_like(raan)], axis=-1)
    v = np.stack([-np.cos(inc) * np.sin(raan), np.cos(inc) * np.cos(raan), np.sin(inc)], axis=-1)
    c, s = np.cos(th)[..., None], np.sin(th)[..., None]
    return R[..., None] * (c * u + s * v), (R * w)[..., None] * (-s * u + c * v)


def trajectories(orb, n, span):
    """The orbits as the library returns trajectories: Y (S, 7, n) in each satellite's own units (length = its radius, time = its
    period), n nodes uniform over span[s] = (t_first, t_last) seconds; units (S, 2)."""
    S = len(orb["R"])
    span = np.broadcast_to(np.asarray(span, dtype=np.float64), (S, 2))
    units = np.column_stack([orb["R"], 2 * np.pi / orbit_rate(orb)])
    t = span[:, :1] + (span[:, 1:] - span[:, :1]) * np.linspace(0.0, 1.0, n)[None, :]          # (S, n)
    o = {k: v[:, None] for k, v in orb.items()}
    p, v = kepler_state(o, t)                                                                   # (S, n, 3)
    Y = np.ones((S, 7, n))
    Y[:, 0:3] = np.transpose(p, (0, 2, 1)) / units[:, 0, None, None]
    Y[:, 3:6] = np.transpose(v, (0, 2, 1)) / (units[:, 0] / units[:, 1])[:, None, None]
    return Y, units, span.copy()


# ---------------------------------------------------------------- the restatement
def grid(M, T0, T1):
    """the common instants: m * h, the last one exactly T1"""
    h = (T1 - T0) / (M - 1)
    t = T0 + np.arange(M) * h
    t[-1] = T1
    return t, h


def ephemeris(Y, units, span, M, T0, T1, ns=None):
    """eph (S, 6, M), status (S,)"""
    Y = np.asarray(Y, dtype=np.float64)
    S, _, n = Y.shape
    t, _ = grid(M, T0, T1)
    eph = np.full((S, 6, M), np.nan)
    status = np.zeros(S, dtype=np.int32)
    for s in range(S):
        nn = n if ns is None else int(ns[s])
        ta, tb = span[s]
        if nn < 2 or nn > n or not tb > ta:
            status[s] = ST_BADK
            continue
        inside = (t >= ta) & (t <= tb)
        if not inside.any():
            continue
        hn = (tb - ta) / (nn - 1)
        u = (t[inside] - ta) / hn
        k = np.clip(u.astype(np.int64), 0, nn - 2)
        sg = u - k
        s2 = sg * sg; s3 = s2 * sg
        h00 = 2.0 * s3 - 3.0 * s2 + 1.0; h10 = s3 - 2.0 * s2 + sg; h01 = -2.0 * s3 + 3.0 * s2; h11 = s3 - s2
        g00 = 6.0 * s2 - 6.0 * sg; g10 = 3.0 * s2 - 4.0 * sg + 1.0; g01 = -6.0 * s2 + 6.0 * sg; g11 = 3.0 * s2 - 2.0 * sg
        L = units[s, 0]; V = L / units[s, 1]
        for c in range(3):
            p0 = Y[s, c, k] * L; p1 = Y[s, c, k + 1] * L
            m0 = hn * (Y[s, 3 + c, k] * V); m1 = hn * (Y[s, 3 + c, k + 1] * V)
            eph[s, c, inside] = h00 * p0 + h10 * m0 + h01 * p1 + h11 * m1
            eph[s, 3 + c, inside] = (g00 * p0 + g10 * m0 + g01 * p1 + g11 * m1) / hn
    return eph, status


def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def _hermite(s, d0, a0, d1, a1):
    s = s[:, None]
    s2 = s * s; s3 = s2 * s
    return (2.0 * s3 - 3.0 * s2 + 1.0) * d0 + (s3 - 2.0 * s2 + s) * a0 + (-2.0 * s3 + 3.0 * s2) * d1 + (s3 - s2) * a1


def pair_minima(eph, T0, T1):
    """For every pair lo < hi (np.triu_indices order): squared minimum distance q (inf: no valid interval), its time, and the
    relative speed there; plus the number of valid intervals and of those that took the Newton steps."""
    eph = np.asarray(eph, dtype=np.float64)
    S, _, M = eph.shape
    lo, hi = np.triu_indices(S, 1)
    t, h = grid(M, T0, T1)
    bad = np.isnan(eph).any(axis=1)                                  # (S, M): an end with a NaN in any of its six values
    P = len(lo)
    best = np.full(P, np.inf); tbest = np.full(P, np.nan)
    n_valid = n_newton = 0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for m in range(M - 1):
            ok = ~(bad[lo, m] | bad[lo, m + 1] | bad[hi, m] | bad[hi, m + 1])
            if not ok.any():
                continue
            l, g = lo[ok], hi[ok]
            d0 = eph[g, 0:3, m] - eph[l, 0:3, m]; d1 = eph[g, 0:3, m + 1] - eph[l, 0:3, m + 1]
            q0 = _dot(d0, d0); q1 = _dot(d1, d1)
            q = q0.copy(); tq = np.full(len(l), t[m])
            sel = q1 < q
            q[sel] = q1[sel]; tq[sel] = t[m + 1]
            D = d1 - d0
            DD = _dot(D, D); b = _dot(d0, D)
            use = (DD > 0.0) & (DD < np.inf)
            s = np.zeros(len(l))
            s[use] = np.clip(-b[use] / DD[use], 0.0, 1.0)
            nt = (s > 0.0) & (s < 1.0)
            n_valid += len(l); n_newton += int(nt.sum())
            if nt.any():
                e0, e1 = d0[nt], d1[nt]
                a0 = h * (eph[g[nt], 3:6, m] - eph[l[nt], 3:6, m]); a1 = h * (eph[g[nt], 3:6, m + 1] - eph[l[nt], 3:6, m + 1])
                sn = s[nt]
                for _ in range(3):
                    x = _hermite(sn, e0, a0, e1, a1)
                    c = sn[:, None]; c2 = c * c
                    x1 = (6.0 * c2 - 6.0 * c) * e0 + (3.0 * c2 - 4.0 * c + 1.0) * a0 + (-6.0 * c2 + 6.0 * c) * e1 + (3.0 * c2 - 2.0 * c) * a1
                    x2 = (12.0 * c - 6.0) * e0 + (6.0 * c - 4.0) * a0 + (-12.0 * c + 6.0) * e1 + (6.0 * c - 2.0) * a1
                    gg = _dot(x, x1); gp = _dot(x1, x1) + _dot(x, x2)
                    step = gp > 0.0
                    sn = np.where(step, np.clip(sn - gg / np.where(step, gp, 1.0), 0.0, 1.0), sn)
                x = _hermite(sn, e0, a0, e1, a1)
                qs = _dot(x, x)
                idx = np.flatnonzero(nt)
                better = qs < q[idx]
                q[idx[better]] = qs[better]; tq[idx[better]] = t[m] + sn[better] * h
            better = q < best[ok]
            at = np.flatnonzero(ok)[better]
            best[at] = q[better]; tbest[at] = tq[better]
    return lo, hi, best, tbest, dict(valid=n_valid, newton=n_newton)


class Screen:
    """dmin, partner, tca per row; pairs (all pairs with a valid interval: rows i, j, d, t sorted by (i, j)); newton_share"""

    def pairs_within(self, threshold):
        return self.pairs[self.pairs[:, 2] <= threshold]


def screen(eph, T0, T1):
    eph = np.asarray(eph, dtype=np.float64)
    S = eph.shape[0]
    lo, hi, q, tq, stats = pair_minima(eph, T0, T1)
    Q = np.full((S, S), np.inf); T = np.full((S, S), np.nan)
    Q[lo, hi] = q; Q[hi, lo] = q; T[lo, hi] = tq; T[hi, lo] = tq
    r = Screen()
    if S > 1:
        j = np.argmin(Q, axis=1)                                     # the first minimum: the smaller partner on a tie
        qmin = Q[np.arange(S), j]
    else:
        j = np.zeros(1, dtype=np.int64); qmin = np.full(1, np.inf)
    none = ~(qmin < np.inf)
    r.dmin = np.where(none, np.inf, np.sqrt(qmin))
    r.partner = np.where(none, -1, j).astype(np.int32)
    r.tca = np.where(none, np.nan, T[np.arange(S), j])
    have = q < np.inf
    r.pairs = np.column_stack([lo[have], hi[have], np.sqrt(q[have]), tq[have]]).astype(np.float64).reshape(-1, 4)
    r.Q = Q
    r.newton_share = stats["newton"] / max(stats["valid"], 1)
    return r


# ---------------------------------------------------------------- shared cases (computed once per shape)
@functools.lru_cache(maxsize=None)
def case(S, M, seed=0, n=40, orbits=1.0):
    """S random LEO orbits over `orbits` revolutions of the lowest one: trajectories with n nodes, their restated ephemeris on M
    instants and its restated screen.  Treat as read-only."""
    orb = random_orbits(S, seed + 1000 * S + M)
    T0, T1 = 0.0, orbits * 2 * np.pi / orbit_rate(orb).max()
    Y, units, span = trajectories(orb, n, (T0 - 1.0, T1 + 1.0))
    eph, status = ephemeris(Y, units, span, M, T0, T1)
    return dict(orb=orb, Y=Y, units=units, span=span, M=M, T0=T0, T1=T1, eph=eph, ref=screen(eph, T0, T1))
