"""numpy restatement of the window probability's thrust sensitivity and of the manoeuvre that aims at it (include/mpcx.h:
mpcx_collision_window_sensitivity, mpcx_avoidance_window) in the header's order of operations: the state gradient c_q of every time
node and of the ball term, the shares it puts on the bracketing node states, the adjoint sweep over A, B_kn, B_kp; the direction, the
unit response through the linearised dynamics, the window rule at the moved means and the step-length search.  The window rule itself,
the objects on their nodes and the scenes come from collision_window_reference, the ordered products and the thrusting arc from
avoidance_reference; nothing of them is copied.  With every result comes an entrywise bound on what two correct fp64 evaluations may
differ by.  Test infrastructure: the product never imports it."""
import numpy as np

import avoidance_reference as AV
import collision_window_reference as CW

ST_OK, ST_SINGULAR, ST_MAXITER, ST_NUMERIC, ST_INFEASIBLE, ST_BADK = 0, 4, 5, 6, 8, 9
NAW = 9
P0, P1, ALPHA, DQ_LINEAR, DV_I, DV_J, UMAX_I, UMAX_J, EVALS = range(NAW)
EPS, GAMMA, POSITION_ALLOWANCE = AV.EPS, AV.GAMMA, AV.POSITION_ALLOWANCE
WHO = AV.WHO


def _ordered_sum(term):
    """term (16, 32, ...) or (64, 2, 32): the sum over the two point axes in the device's order (numpy's cumsum adds one by one)"""
    if term.shape[0] == 64:
        return np.cumsum(term.reshape(64, -1), axis=1)[:, -1]
    return np.cumsum(term.reshape((-1,) + term.shape[2:]), axis=0)[-1]


def _unwhiten(Li, u):
    """L^-T u"""
    i00, i10, i11, i20, i21, i22 = Li
    return np.array([i00 * u[0] + i10 * u[1] + i20 * u[2], i11 * u[1] + i21 * u[2], i22 * u[2]])


def rate_and_gradient(R, d, w, A, B, D, wf=None, grad=True):
    """cw_rate_grad at every node: d, w (3, T) the means, [[A, B^T], [B, D]] the covariance, wf the velocity that places the sphere
    rule's pole (w itself when None) -> ok (T,), rate (T,) [, cg (6, T) = (d rate / dd | d rate / dw), cabs (6, T) the same sums over
    the terms' magnitudes].  The rate is collision_window_reference.entry_rate's, expression for expression."""
    from scipy.special import erfc
    _, ew, e1, e2 = CW.sphere_frame(w if wf is None else wf)
    ok, Li, W, Sc, cden = CW.node_setup(A, B, D)
    with np.errstate(all="ignore"):
        wq, n = CW.sphere_points(np.arange(CW.NMU), ew, e1, e2)
        z = CW.whitened(n, R, d, Li)
        z0, z1, z2 = z
        dens = np.exp(-0.5 * (z0 * z0 + z1 * z1 + z2 * z2))
        v0 = (n[0] * (w[0] + (W[0, 0] * z0 + W[0, 1] * z1 + W[0, 2] * z2)) + n[1] * (w[1] + (W[1, 0] * z0 + W[1, 1] * z1 + W[1, 2] * z2))
              + n[2] * (w[2] + (W[2, 0] * z0 + W[2, 1] * z1 + W[2, 2] * z2)))
        s2 = (n[0] * (Sc[0] * n[0] + Sc[1] * n[1] + Sc[2] * n[2]) + n[1] * (Sc[1] * n[0] + Sc[3] * n[1] + Sc[4] * n[2])
              + n[2] * (Sc[2] * n[0] + Sc[4] * n[1] + Sc[5] * n[2]))
        pos = s2 > 0.0
        s = np.sqrt(np.where(pos, s2, 1.0))
        a = v0 / s
        Phi = np.where(pos, 0.5 * erfc(a * CW.INV_SQRT2), np.where(v0 < 0.0, 1.0, 0.0))
        E = np.where(pos, s * (np.exp(-0.5 * a * a) * CW.INV_SQRT_2PI) - v0 * Phi, np.maximum(-v0, 0.0))
        sc = (R * R) * cden
        rate = sc * _ordered_sum(wq[..., None] * (dens * E))
        if not grad:
            return ok, rate
        wd = wq[..., None] * dens
        wp = wd * Phi
        Wn = [W[0, b] * n[0] + W[1, b] * n[1] + W[2, b] * n[2] for b in range(3)]
        u = [_ordered_sum(wd * (E * z[b] + Phi * Wn[b])) for b in range(3)]
        v = [_ordered_sum(wp * n[c]) for c in range(3)]
        gd = _unwhiten(Li, u)
        cg = np.array([sc * gd[0], sc * gd[1], sc * gd[2], -(sc * v[0]), -(sc * v[1]), -(sc * v[2])])
        ua = [_ordered_sum(wd * (E * np.abs(z[b]) + Phi * np.abs(Wn[b]))) for b in range(3)]
        va = [_ordered_sum(wp * np.abs(n[c])) for c in range(3)]
        ga = _unwhiten([np.abs(x) for x in Li], ua)
        cabs = np.array([sc * ga[0], sc * ga[1], sc * ga[2], sc * va[0], sc * va[1], sc * va[2]])
    return ok, rate, cg, cabs


def ball_and_gradient(R, d, w, A, grad=True):
    """cw_ball_share_grad over the 64 lanes and the butterfly: P(|rho| <= R) for rho ~ N(d, A), the pole along w -> ok, start
    [, gb (3,) = d start / dd, gabs (3,)].  start is collision_window_reference.ball_probability's, expression for expression."""
    _, ew, e1, e2 = CW.sphere_frame(w[:, None])
    A3 = A[:, :, None]
    ok, Li, _, _, cden = CW.node_setup(A3, np.zeros_like(A3), np.zeros_like(A3))
    Li = [x[0] for x in Li]
    lane = np.arange(64)
    i, j0 = lane >> 3, 2 * (lane & 7)
    with np.errstate(all="ignore"):
        r = R * (0.5 + 0.5 * CW.GL8_X[i])
        wr = ((0.5 * R) * CW.GL8_W[i]) * (r * r)
        wq, n = CW.sphere_points(np.stack([j0, j0 + 1], axis=1), ew[:, 0], e1[:, 0], e2[:, 0])
        z = CW.whitened(n, r[:, None, None], d, Li)
        term = wq * np.exp(-0.5 * (z[0] * z[0] + z[1] * z[1] + z[2] * z[2]))
        start = float(cden[0] * CW.butterfly_sum(wr * _ordered_sum(term)))
        if not grad:
            return bool(ok[0]), start
        gz = [CW.butterfly_sum(wr * _ordered_sum(term * z[b])) for b in range(3)]
        ga = [CW.butterfly_sum(wr * _ordered_sum(term * np.abs(z[b]))) for b in range(3)]
        gb = cden[0] * _unwhiten(Li, gz)
        gabs = cden[0] * _unwhiten([abs(x) for x in Li], ga)
    return bool(ok[0]), start, gb, gabs


def bases(side, o, tau):
    """cw_basis of object o of side = (Y, units, span, P, radius, ns) at the times tau (T,): the interval k (T,) and how position (m)
    and velocity (m/s) depend on (y_pos[k], y_vel[k], y_pos[k+1], y_vel[k+1]) in normalised units: bp, bv (4, T)"""
    Y, units, span, _, _, ns = side
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
    L, Tu = units[o]
    V = L / Tu
    htau = ((tb - ta) / Tu) / (nn - 1)
    bp = np.array([L * h00, L * (htau * h10), L * h01, L * (htau * h11)])
    bv = np.array([(L * g00) / hn, V * g10, (L * g01) / hn, V * g11])
    return k, bp, bv


def state_gradient(R, ta, tb, panels, state):
    """The c_q of one row: state(tau) -> (d, w, A, B, D) -> ok, tau (64 panels + 1,) (the last one t_a: the ball term), c (64 panels
    + 1, 6), Ec its entrywise bound, start, entries.  Bound: the terms of c_q are the rate's terms times a factor linear in z or n
    and as many multiply-adds again, so they get twice collision_window_reference.rounding_bound relative to the sum of their
    magnitudes; beside that the Hermite positions' 2e-7 m move z by 2e-7 / sigma_min, which the factor z passes on absolutely: the
    node's weighted rate times |L^-T| 1 times that."""
    hp = (tb - ta) / panels
    taus, cs, mags, rates = [], [], [], []
    entries, dg = 0.0, {}
    for p in range(panels):
        tau = (ta + p * hp) + (0.5 * hp) * (1.0 + CW.GL_X)
        d, w, A, B, D = state(tau)
        ok, rate, cg, cabs = rate_and_gradient(R, d, w, A, B, D)
        if not ok.all():
            return False, None, None, None, np.nan, np.nan
        CW._diagnose(dg, d, A)
        om = (0.5 * hp) * CW.GL_W
        entries = entries + CW.butterfly_sum(om * rate)
        still = ~(d.any(axis=0) | w.any(axis=0))                         # d = w = 0 exactly: the derivative is 0 by symmetry
        taus.append(tau); cs.append(np.where(still[:, None], 0.0, (om * cg).T)); mags.append(np.where(still[:, None], 0.0, (om * cabs).T))
        rates.append((om * rate)[:, None] * _lit_row_sums(A))
    d, w, A, _, _ = state(np.array([ta]))
    ok, start, gb, gabs = ball_and_gradient(R, d[:, 0], w[:, 0], A[:, :, 0])
    if not ok:
        return False, None, None, None, np.nan, np.nan
    rho = 2.0 * CW.rounding_bound(R, dg)
    shift = POSITION_ALLOWANCE / dg["sigma_min"]
    if not d.any():                                                      # the ball about the mean: 0 by symmetry
        gb, gabs = np.zeros(3), np.zeros(3)
    c = np.concatenate(cs + [np.concatenate([gb, np.zeros(3)])[None]])
    Ec = rho * np.concatenate(mags + [np.concatenate([gabs, np.zeros(3)])[None]])
    Ec[:, :3] += shift * np.concatenate(rates + [start * _lit_row_sums(A)])
    return True, np.concatenate(taus + [np.array([ta])]), c, Ec, start, entries


def _lit_row_sums(A):
    """|L^-T| 1 for A (3, 3, T) = L L^T -> (T, 3)"""
    Lc = np.linalg.cholesky(np.transpose(A, (2, 0, 1)))
    return np.abs(np.transpose(np.linalg.inv(Lc), (0, 2, 1))).sum(axis=2)


def sources(side, o, sgn, taus, c, Ec, K):
    """The node sources of one object: every c_q's shares on its two bracketing node states, summed over q in ascending order
    -> sigma (K, 7), its bound, ke (the interval of the last time node; the ball term's is not later).  Bound: the bases are O(1)
    polynomials times the units, good to 8 eps of the units' scale; a sum of up to 64 panels + 1 terms."""
    k, bp, bv = bases(side, o, taus)
    sig, Es = np.zeros((K, 7)), np.zeros((K, 7))
    L, Tu = side[1][o]
    unit_p, unit_v = 8 * EPS * abs(L), 8 * EPS * abs(L / Tu) * max(1.0, float(np.abs(bv).max() / max(abs(L / Tu), 1e-300)))
    n_terms = (len(taus) + 8) * EPS
    for x in (2, 0, 3, 1):                                               # a node gets the upper shares of the interval before it first: q ascends
        m, cols = k + (x >> 1), slice(3 * (x & 1), 3 * (x & 1) + 3)
        pos, vel = c[:, :3] * bp[x][:, None], c[:, 3:] * bv[x][:, None]
        np.add.at(sig[:, cols], m, sgn * (pos + vel))                    # (one by one, in the order of q)
        np.add.at(Es[:, cols], m, Ec[:, :3] * np.abs(bp[x])[:, None] + Ec[:, 3:] * np.abs(bv[x])[:, None] + np.abs(c[:, :3]) * unit_p
                  + np.abs(c[:, 3:]) * unit_v + n_terms * (np.abs(pos) + np.abs(vel)))
    return sig, Es, int(k[:-1].max())


def sweep(A, Bn, Bp, sig, ke, K, Esig=None):
    """lam_ke+1 = sigma_ke+1, lam_m = lam_m+1 A_m + sigma_m; g_m = lam_m+1 B_kn[m] (m <= ke) + lam_m B_kp[m-1] (1 <= m <= ke + 1)
    -> g (3, K) [, its bound in the manner of avoidance_reference.sweep_error_bound when Esig is given]"""
    lam = {ke + 1: sig[ke + 1][None]}
    for m in range(ke, -1, -1):
        lam[m] = AV.ordered(lam[m + 1], A[m]) + sig[m][None]
    g = np.zeros((3, K))
    for m in range(0, ke + 2):
        if m <= ke and m >= 1:
            g[:, m] = (AV.ordered(lam[m + 1], Bn[m]) + AV.ordered(lam[m], Bp[m - 1]))[0]
        elif m <= ke:
            g[:, m] = AV.ordered(lam[m + 1], Bn[m])[0]
        else:
            g[:, m] = AV.ordered(lam[m], Bp[m - 1])[0]
    if Esig is None:
        return g
    aA, aBn, aBp = np.abs(A), np.abs(Bn), np.abs(Bp)
    E = {ke + 1: Esig[ke + 1][None]}
    mag = {ke + 1: np.abs(sig[ke + 1][None])}                            # the magnitude the products run through (sources may cancel)
    for m in range(ke, -1, -1):
        mag[m] = mag[m + 1] @ aA[m] + np.abs(sig[m][None])
        E[m] = E[m + 1] @ aA[m] + GAMMA * mag[m] + Esig[m][None]
    Eg = np.zeros((3, K))
    for m in range(0, ke + 2):
        if m <= ke:
            Eg[:, m] += (E[m + 1] @ aBn[m] + GAMMA * (mag[m + 1] @ aBn[m]))[0]
        if m >= 1:
            Eg[:, m] += (E[m] @ aBp[m - 1] + GAMMA * (mag[m] @ aBp[m - 1]))[0]
    return g, Eg


def _row_setup(rows, cols, fi, fj, t, h):
    """the window call's tests of one row -> (status, oa, ob, ta, tb, R)"""
    st, oa, sa = CW._object_check(rows, fi, t)
    if st == ST_OK:
        st, ob, sb = CW._object_check(cols, fj, t)
    if st == ST_OK and not (h > 0.0 and np.isfinite(h)):
        st = ST_BADK
    if st != ST_OK:
        return st, None, None, None, None, None
    ta = max(max(t - h, sa[0]), sb[0]); tb = min(min(t + h, sa[1]), sb[1])
    if not tb > ta:
        return ST_BADK, None, None, None, None, None
    R = float(rows[4][oa]) + float(cols[4][ob])
    return (ST_OK if np.isfinite(R) else ST_NUMERIC), oa, ob, ta, tb, R


def _mover_status(rows, o, disc_status):
    span, units = rows[2], rows[1]
    with np.errstate(all="ignore"):
        tf = (span[o, 1] - span[o, 0]) / np.float64(units[o, 1])
    if not tf > 0.0 or not np.isfinite(tf):
        return ST_BADK
    if disc_status is not None and disc_status[o] != 0:
        return int(disc_status[o])
    return ST_OK


def row_gradients(pairs, rows, half_window, panels, cols=None, mu=CW.MU_EARTH):
    """What does not depend on who moves, row for row: a list of dicts (st, oa, ob, ta, tb, R and, for a good row with a sphere, tau,
    c, Ec, start, entries).  Computed once per scene and panel count and shared by every form of the list."""
    pairs = np.asarray(pairs, dtype=np.float64).reshape(-1, 4)
    cols = rows if cols is None else cols
    hw = np.broadcast_to(np.asarray(half_window, dtype=np.float64), (len(pairs),))
    res = []
    for r, (fi, fj, _, t) in enumerate(pairs):
        st, oa, ob, ta, tb, R = _row_setup(rows, cols, fi, fj, t, hw[r])
        e = dict(st=st, oa=oa, ob=ob, ta=ta, tb=tb, R=R)
        if st == ST_OK and R > 0.0:
            ok, tau, c, Ec, start, entries = state_gradient(R, ta, tb, panels, lambda tt: CW.relative_state(rows, cols, oa, ob, tt, mu))
            if not ok or not np.isfinite(start + entries):
                e["st"] = ST_NUMERIC
            else:
                e.update(tau=tau, c=c, Ec=Ec, start=start, entries=entries)
        res.append(e)
    return res


def window_sensitivity(grads, rows, stage, who="i", cols=None, disc_status=None):
    """grads: row_gradients of the list; rows, cols = (Y, units, span, P, radius, ns) (cols None: the columns are the rows); stage =
    (A (S, K-1, 7, 7), Bn = B_kn, Bp = B_kp (S, K-1, 7, 3)) -> sens (n, NS, 3, K), its entrywise bound, status (n,)"""
    A, Bn, Bp = stage
    K = rows[0].shape[2]
    who = WHO[who] if isinstance(who, str) else who
    NS = 1 if cols is not None else 2
    moves = (who != 1, NS == 2 and who != 0)
    n = len(grads)
    sens, Es, status = np.full((n, NS, 3, K), np.nan), np.zeros((n, NS, 3, K)), np.zeros(n, dtype=np.int32)
    for r, e in enumerate(grads):
        st = e["st"]
        if st == ST_OK and not e["R"] > 0.0:
            sens[r] = 0.0
            continue
        obj = (e["oa"], e["ob"])
        for sl in (0, 1):
            if st == ST_OK and moves[sl]:
                st = _mover_status(rows, obj[sl], disc_status)
        if st == ST_OK:
            sens[r] = 0.0
            for sl in (0, 1):
                if not moves[sl]:
                    continue
                o = obj[sl]
                sig, Esig, ke = sources(rows, o, 1.0 if sl else -1.0, e["tau"], e["c"], e["Ec"], K)
                sens[r, sl], Es[r, sl] = sweep(A[o], Bn[o], Bp[o], sig, ke, K, Esig)
        status[r] = st
    return sens, Es, status


# ---------------------------------------------------------------- the manoeuvre
def direction(rows, g, objs, moves, K):
    """da_m = -ghat_m / w_m, the unit step du = da_m / c_m, Gamma, and per object sum w |da| and max |du| -> du1 (NS, 3, K), Gamma,
    dv (2,), umax (2,)"""
    Y, units, span, _, _, ns = rows
    NS = g.shape[0]
    du1, Gam, dv, um = np.zeros((NS, 3, K)), 0.0, np.zeros(2), np.zeros(2)
    for sl in range(NS):
        if not moves[sl]:
            continue
        o = objs[sl]
        nn = K if ns is None else int(ns[o])
        L, Tu = units[o]
        hn = (span[o, 1] - span[o, 0]) / (nn - 1)
        cm = (L / (Tu * Tu)) / Y[o, 6, :nn]
        wm = AV.node_weights(hn, nn, K)[:nn]
        gh = g[sl][:, :nn] / cm
        da = -gh / wm
        du1[sl][:, :nn] = da / cm
        Gam = Gam + ((gh * gh).sum(axis=0) / wm).sum()
        dv[sl] = (wm * np.sqrt((da * da).sum(axis=0))).sum()
        um[sl] = np.sqrt((du1[sl] * du1[sl]).sum(axis=0)).max()
    return du1, Gam, dv, um


def response(A, Bn, Bp, du, nn):
    """dx_0 = 0, dx_k+1 = A_k dx_k + B_kn[k] du_k + B_kp[k] du_k+1 -> dx (nn, 7)"""
    dx = np.zeros((nn, 7))
    for k in range(nn - 1):
        dx[k + 1] = AV.ordered(A[k], dx[k][:, None])[:, 0] + AV.ordered(Bn[k], du[:, k][:, None])[:, 0] + AV.ordered(Bp[k], du[:, k + 1][:, None])[:, 0]
    return dx


def shifted_window(e, rows, cols, movers, panels, mu=CW.MU_EARTH):
    """Q(alpha) of a row: movers = [(side, object, sgn, dx (nn, 7))] -> a function alpha -> START + ENTRIES of the window rule at the
    means (d + alpha dd, w + alpha dw) with the unmoved frames and covariances"""
    def mean_shift(tau):
        dd, dw = np.zeros((3, len(tau))), np.zeros((3, len(tau)))
        for side, o, sgn, dx in movers:
            k, bp, bv = bases(side, o, tau)
            x0, x1 = dx[k].T, dx[k + 1].T
            dd = dd + sgn * (bp[0] * x0[0:3] + bp[1] * x0[3:6] + bp[2] * x1[0:3] + bp[3] * x1[3:6])
            dw = dw + sgn * (bv[0] * x0[0:3] + bv[1] * x0[3:6] + bv[2] * x1[0:3] + bv[3] * x1[3:6])
        return dd, dw

    ta, tb, R = e["ta"], e["tb"], e["R"]
    hp = (tb - ta) / panels
    nodes = []                                                           # what does not depend on alpha, formed once
    for p in list(range(panels)) + [None]:
        tau = np.array([ta]) if p is None else (ta + p * hp) + (0.5 * hp) * (1.0 + CW.GL_X)
        nodes.append(CW.relative_state(rows, cols, e["oa"], e["ob"], tau, mu) + mean_shift(tau))

    def Q(alpha):
        entries = 0.0
        for d, w, A, B, D, dd, dw in nodes[:-1]:
            _, rate = rate_and_gradient(R, d + alpha * dd, w + alpha * dw, A, B, D, wf=w, grad=False)
            entries = entries + CW.butterfly_sum(((0.5 * hp) * CW.GL_W) * rate)
        d, w, A, _, _, dd, dw = nodes[-1]
        _, start = ball_and_gradient(R, (d + alpha * dd)[:, 0], w[:, 0], A[:, :, 0], grad=False)
        return start + entries
    return Q


def step_length(Q, Q0, Gam, target_p, tol, max_eval):
    """The header's search -> (status, alpha, Q(alpha), evaluations)"""
    f0 = np.log(Q0 / target_p)
    lo, flo, hi, fhi, alpha, evals = 0.0, f0, 0.0, 0.0, Q0 * f0 / Gam, 0
    while True:
        if evals == max_eval:
            return ST_INFEASIBLE, np.nan, np.nan, evals
        Q1 = Q(alpha); evals += 1
        if not Q1 >= 0.0 or not np.isfinite(Q1) or not np.isfinite(alpha):
            return ST_NUMERIC, np.nan, np.nan, evals
        with np.errstate(divide="ignore"):
            f = np.log(Q1 / target_p)
        if abs(f) <= tol:
            return ST_OK, alpha, Q1, evals
        if f <= 0.0:
            hi, fhi = alpha, f
            break
        lo, flo = alpha, f
        alpha = 2.0 * alpha
    side = 0
    while True:
        if evals == max_eval:
            return ST_MAXITER, np.nan, np.nan, evals
        with np.errstate(all="ignore"):
            alpha = lo + (hi - lo) * (flo / (flo - fhi))
        if not (alpha > lo and alpha < hi):
            alpha = 0.5 * (lo + hi)
        Q1 = Q(alpha); evals += 1
        if not Q1 >= 0.0 or not np.isfinite(Q1):
            return ST_NUMERIC, np.nan, np.nan, evals
        with np.errstate(divide="ignore"):
            f = np.log(Q1 / target_p)
        if abs(f) <= tol:
            return ST_OK, alpha, Q1, evals
        if f > 0.0:
            lo, flo = alpha, f
            if side == 1:
                fhi = 0.5 * fhi
            side = 1
        else:
            hi, fhi = alpha, f
            if side == -1:
                flo = 0.5 * flo
            side = -1


def avoidance_window(grads, sens, Es, status, rows, stage, target_p, tol, max_eval, panels, who="i", cols=None, mu=CW.MU_EARTH, only=None):
    """grads, (sens, Es, status) = row_gradients and window_sensitivity of the list -> out (n, NAW), du (n, NS, 3, K), status, and the
    bounds (Eo, Ed).  only: the rows to restate (the others are NaN with status -1).
    Bounds.  Two correct searches may stop at different alpha, each with |ln(Q / target_p)| <= tol: alpha is pinned to 2 tol over
    the slope |d ln Q / d alpha| there (measured by a one-sided difference of 1e-3 alpha), plus what the rounding of Q -- rho =
    collision_window_reference.rounding_bound -- and of the direction -- rel, the sensitivities' bound relative to their largest
    entry -- move the root by; du, DV, UMAX and DQ_LINEAR scale with alpha and the direction; P1 is within 2 tol + rho of itself."""
    A, Bn, Bp = stage
    K = rows[0].shape[2]
    ns = rows[5]
    whoi = WHO[who] if isinstance(who, str) else who
    NS = 1 if cols is not None else 2
    moves = (whoi != 1, NS == 2 and whoi != 0)
    cside = rows if cols is None else cols
    n = len(grads)
    out, du, stat = np.full((n, NAW), np.nan), np.full((n, NS, 3, K), np.nan), np.array(status, dtype=np.int32)
    Eo, Ed = np.zeros((n, NAW)), np.zeros((n, NS, 3, K))
    for r, e in enumerate(grads):
        if only is not None and r not in only:
            stat[r] = -1
            continue
        if stat[r] != ST_OK:
            continue
        Q0 = (e["start"] + e["entries"]) if e["R"] > 0.0 else 0.0
        if Q0 <= target_p:
            out[r] = 0.0; out[r, [P0, P1]] = Q0; du[r] = 0.0
            continue
        objs = (e["oa"], e["ob"])
        du1, Gam, dv, um = direction(rows, sens[r], objs, moves, K)
        if not Gam > 0.0 or not np.isfinite(Gam):
            stat[r] = ST_SINGULAR
            continue
        movers = []
        for sl in range(NS):
            if moves[sl]:
                o = objs[sl]
                nn = K if ns is None else int(ns[o])
                movers.append((rows, o, 1.0 if sl else -1.0, response(A[o], Bn[o], Bp[o], du1[sl], nn)))
        Q = shifted_window(e, rows, cside, movers, panels, mu)
        st, alpha, Q1, evals = step_length(Q, Q0, Gam, target_p, tol, max_eval)
        stat[r] = st
        if st != ST_OK:
            continue
        du[r] = alpha * du1
        out[r] = [Q0, Q1, alpha, -(alpha * Gam), alpha * dv[0], alpha * dv[1], alpha * um[0], alpha * um[1], evals]
        dg = {}
        d, _, A_, _, _ = CW.relative_state(rows, cside, e["oa"], e["ob"], e["tau"][:-1], mu)
        CW._diagnose(dg, d, A_)
        rho = CW.rounding_bound(e["R"], dg)
        rel = max(float((Es[r, sl] / max(np.abs(sens[r, sl]).max(), 1e-300)).max()) for sl in range(NS) if moves[sl]) + 64 * EPS * K
        slope = abs(np.log(Q(alpha * 1.001) / Q1)) / (1e-3 * alpha)
        Ea = (2.0 * tol + 4.0 * rho + 4.0 * rel * abs(np.log(Q0 / Q1))) / slope + 4.0 * rel * alpha
        ra = Ea / alpha + 2.0 * rel
        Ed[r] = ra * np.abs(du[r]).max()
        Eo[r] = np.array([rho * Q0, (2.0 * tol + 2.0 * rho) * Q1, Ea, (ra + 2.0 * rel) * alpha * Gam, ra * alpha * dv[0], ra * alpha * dv[1],
                          ra * alpha * um[0], ra * alpha * um[1], np.inf])
    return out, du, stat, (Eo, Ed)
