"""numpy restatement of the covariance chain with an uncertain drag (include/mpcx.h: mpcx_covariance_drag_batch) -- the same formulas in
the same order as csrc/covariance_drag.hip, on top of covariance_thrust_reference.py -- with the entrywise rounding bound run along the
chain, and the drag column G_k of a stage record (MPCX_FLAG_DRAG_COLUMN) from the CPU oracle's dumped quadrature nodes.  Test
infrastructure: the product never imports it."""
import numpy as np

import collision_reference as C
import covariance_thrust_reference as T

ST_OK, ST_NUMERIC, ST_BADK = T.ST_OK, T.ST_NUMERIC, T.ST_BADK
NDENS = 2
EPS = T.EPS
_trapezoid = getattr(np, "trapezoid", None) or np.trapz                               # (numpy 2 renamed it)


def drag_forcing(y, tf, cst, flags, atmosphere=None):
    """tf [0; a_D(y); 0]: the oracle's dynamics with drag minus its dynamics without.  The difference is taken where nothing but the drag
    is in the acceleration -- mu = 0, no J2, no thrust: the drag depends on none of them -- so that it does not cancel eight digits of
    an acceleration that is 1e8 times the drag (then the difference would carry 1e-8 of its own size in rounding)."""
    import oracle_lib as O
    bare = np.array(cst, dtype=np.float64)
    bare[0] = 0.0                                                                     # MPCX_C_MU
    with_drag, rc1 = O.dynamics(y, np.zeros(3), tf, bare, O.FLAG_DRAG, atmosphere)
    without, rc0 = O.dynamics(y, np.zeros(3), tf, bare, 0)
    assert rc0 == 0 and rc1 == 0
    return with_drag - without


def drag_column(x, u, tf, cst, flags, atmosphere=None, max_step=1e-2):
    """G (K-1, 7), G_k = d x_k+1 / d beta = A_k trapz(Phi(tau)^-1 tf [0; a_D; 0]) over the accepted nodes of the oracle's discretisation of
    (x (7, K), u (3, K), tf) under flags (FLAG_DRAG among them) and atmosphere: at every dumped node Phi^-1 times the drag forcing,
    numpy's trapezoid over the interval's nodes, then A_k @.  -> (G, the oracle's discretisation)"""
    import oracle_lib as O
    assert flags & O.FLAG_DRAG
    d = O.discretize(x, u, tf, cst, flags, max_step, dump_nodes=True, atmosphere=atmosphere, node_rows=1024)     # (K = 2: 100 steps and more)
    assert d["status"] == 0
    ends = np.concatenate([[0], np.cumsum(d["node_counts"])])
    G = np.zeros((x.shape[1] - 1, 7))
    for k in range(x.shape[1] - 1):
        t, ys = d["node_t"][ends[k]:ends[k + 1]], d["node_y"][ends[k]:ends[k + 1]]
        g = np.array([np.linalg.solve(y[:49].reshape(7, 7), drag_forcing(y[49:], tf, cst, flags, atmosphere)) for y in ys])
        G[k] = d["A"][k] @ _trapezoid(g, t, axis=0)
    return G, d


def phi_beta(h, tau):
    """phi = exp(-h / tau_b) of a node spacing of h seconds: exactly 1 for tau_b = inf"""
    return np.exp(-h / tau)


def phi8(A, Gk, L, Tu, ph):
    """[[D A D^-1, D G], [0, phi]], D = diag(L, L, L, V, V, V, 1)"""
    out = np.zeros((8, 8))
    out[:7, :7] = T.physical_phi7(A, L, Tu)
    out[:7, 7] = np.array([L] * 3 + [L / Tu] * 3 + [1.0]) * np.asarray(Gk, dtype=np.float64)
    out[7, 7] = ph
    return out


def drag_step(p8, bn, bp, P8, Cx, Sk, Sk1, noise8):
    """one interval: (((((Phi8 P8) Phi8^T + (Y + Y^T)) + (Bn Sigma_k) Bn^T) + (Bp Sigma_k+1) Bp^T) + noise, the thrust terms on the 7 x 7
    block, the sums over the state in ascending order (the beta term last), upper triangle mirrored; and C_k+1 = Bp Sigma_k+1"""
    op = C._ordered_product
    N = op(op(p8, P8), p8.T)
    Y = op(op(p8[:7, :7], Cx), bn.T)
    BT = op(bp, Sk1)
    N7 = ((N[:7, :7] + (Y + Y.T)) + op(op(bn, Sk), bn.T)) + op(BT, bp.T)
    N = N.copy(); N[:7, :7] = N7
    return T._mirror(N + noise8), BT


def _rows(density, S):
    return np.broadcast_to(np.asarray(density, dtype=np.float64), (S, NDENS))


def covariance_drag_chain(A, Bn, Bp, G, U, units, span, P0, density, execution=None, q=None, m_var0=None, ns=None, disc_status=None):
    """A (S, K-1, 7, 7), Bn, Bp (S, K-1, 7, 3), G (S, K-1, 7) the stage records' blocks with the drag column, U (S, 3, K), density
    (S, 2) = (sigma_b, tau_b)  ->  P (S, K, 6, 6), Pm (S, K, 7), Pb (S, K, 8), status (S,)"""
    A = np.asarray(A, dtype=np.float64)
    S, K = A.shape[0], A.shape[1] + 1
    P0 = np.broadcast_to(np.asarray(P0, dtype=np.float64), (S, 6, 6))
    execution = np.broadcast_to(np.zeros(T.NEXEC) if execution is None else np.asarray(execution, dtype=np.float64), (S, T.NEXEC))
    mv = np.zeros(S) if m_var0 is None else np.broadcast_to(np.asarray(m_var0, dtype=np.float64), (S,))
    density = _rows(density, S)
    P, Pm, Pb = np.zeros((S, K, 6, 6)), np.zeros((S, K, 7)), np.zeros((S, K, 8))
    status = np.zeros(S, dtype=np.int32)
    iu = np.triu_indices(6)
    for s in range(S):
        nn = K if ns is None else int(ns[s])
        ta, tb = span[s]
        L, Tu = units[s]
        p0 = np.empty((6, 6)); p0[iu] = P0[s][iu]; p0.T[iu] = P0[s][iu]
        ex, (sb, tau) = execution[s], density[s]
        with np.errstate(all="ignore"):
            tf = (tb - ta) / np.float64(Tu)
        if nn < 2 or nn > K or not tb > ta or not tf > 0.0 or not np.isfinite(tf):
            status[s] = ST_BADK
        elif disc_status is not None and disc_status[s] != 0:
            status[s] = disc_status[s]
        elif not np.isfinite(p0).all():
            status[s] = ST_NUMERIC
        elif not (np.isfinite(ex).all() and (ex >= 0.0).all() and np.isfinite(mv[s]) and mv[s] >= 0.0):
            status[s] = ST_NUMERIC
        elif not (np.isfinite(sb) and sb >= 0.0 and tau > 0.0):
            status[s] = ST_NUMERIC
        if status[s]:
            P[s] = np.nan; Pm[s] = np.nan; Pb[s] = np.nan
            continue
        h = (tb - ta) / (nn - 1)
        ph = phi_beta(h, tau)
        noise8 = np.zeros((8, 8))
        noise8[:6, :6] = (0.0 if q is None else float(np.broadcast_to(q, (S,))[s])) * C.q_matrix(h)
        noise8[7, 7] = (1.0 - ph * ph) * (sb * sb)
        P8 = np.zeros((8, 8)); P8[:6, :6] = p0; P8[6, 6] = mv[s]; P8[7, 7] = sb * sb
        Cx = np.zeros((7, 3))
        P[s, 0] = P8[:6, :6]; Pm[s, 0] = P8[6, :7]; Pb[s, 0] = P8[7]
        Sk = T.sigma(U[s, :, 0], ex)
        for k in range(nn - 1):
            Sk1 = T.sigma(U[s, :, k + 1], ex)
            p8 = phi8(A[s, k], G[s, k], L, Tu, ph)
            P8, Cx = drag_step(p8, T.physical_b(Bn[s, k], L, Tu), T.physical_b(Bp[s, k], L, Tu), P8, Cx, Sk, Sk1, noise8)
            P[s, k + 1] = P8[:6, :6]; Pm[s, k + 1] = P8[6, :7]; Pb[s, k + 1] = P8[7]
            Sk = Sk1
    return P, Pm, Pb, status


def chain_error_bound(A, Bn, Bp, G, U, units, span, P0, density, execution=None, q=None, m_var0=None, ns=None, gamma=32 * EPS):
    """covariance_thrust_reference.chain_error_bound extended by the beta row and column: the standard bound of floating-point
    products run along the chain of MAGNITUDES, now 8 x 8.  With a = |Phi8| (|Phi~|, |G~| and phi), n = |Bn~|, p = |Bp~| (a zero beta
    row), M_k an entrywise bound of |P8_k| and its summands, G_k of |C_k|:
        E_k+1 = a E_k a^T + (a F_k n^T + its transpose) + gamma (a M_k a^T + (a G_k n^T + its transpose) + n |S_k| n^T + p |S_k+1| p^T
                                                                  + w e_7 e_7^T)
        F_k+1 = gamma p |S_k+1|,        w = (1 + phi^2) sigma_b^2.
    gamma = 32 eps covers, per entry, what it covers there with the sums one term longer (two eight-term products: 16 eps), forming
    G~ (1 eps), and phi: the exponential is correct to a few ulp on either side (taken as 4 eps of phi: 8 eps of phi^2 -- in a M a^T
    through a's entry phi, and in the noise (1 - phi^2) sigma_b^2 through w, which also bounds that entry's own three roundings).
    -> E (S, K, 6, 6), Em (S, K, 7), Eb (S, K, 8), entrywise bounds for P, Pm and Pb."""
    S, K = A.shape[0], A.shape[1] + 1
    execution = np.broadcast_to(np.zeros(T.NEXEC) if execution is None else np.asarray(execution, dtype=np.float64), (S, T.NEXEC))
    mv = np.zeros(S) if m_var0 is None else np.broadcast_to(np.asarray(m_var0, dtype=np.float64), (S,))
    P0 = np.broadcast_to(np.asarray(P0, dtype=np.float64), (S, 6, 6))
    density = _rows(density, S)
    E, Em, Eb = np.zeros((S, K, 6, 6)), np.zeros((S, K, 7)), np.zeros((S, K, 8))
    for s in range(S):
        nn = K if ns is None else int(ns[s])
        L, Tu = units[s]
        sb, tau = density[s]
        h = (span[s, 1] - span[s, 0]) / (nn - 1)
        ph = phi_beta(h, tau)
        M = np.zeros((8, 8)); M[:6, :6] = np.abs(np.triu(P0[s]) + np.triu(P0[s], 1).T); M[6, 6] = mv[s]; M[7, 7] = sb * sb
        noise8 = np.zeros((8, 8)); noise8[:6, :6] = (0.0 if q is None else float(np.broadcast_to(q, (S,))[s])) * C.q_matrix(h)
        noise8[7, 7] = (1.0 - ph * ph) * (sb * sb)
        w8 = np.zeros((8, 8)); w8[7, 7] = (1.0 + ph * ph) * (sb * sb)
        E8, F, Gm = np.zeros((8, 8)), np.zeros((8, 3)), np.zeros((8, 3))
        Sk = T.sigma_magnitude(U[s, :, 0], execution[s])
        for k in range(nn - 1):
            Sk1 = T.sigma_magnitude(U[s, :, k + 1], execution[s])
            a = np.abs(phi8(A[s, k], G[s, k], L, Tu, ph))
            n, p = np.zeros((8, 3)), np.zeros((8, 3))
            n[:7] = np.abs(T.physical_b(Bn[s, k], L, Tu)); p[:7] = np.abs(T.physical_b(Bp[s, k], L, Tu))
            a7 = a.copy(); a7[:, 7] = 0.0; a7[7] = 0.0                      # (C has no beta row: Phi~ alone carries it)
            aGn, aFn = a7 @ Gm @ n.T, a7 @ F @ n.T
            Mn = a @ M @ a.T + (aGn + aGn.T) + n @ Sk @ n.T + p @ Sk1 @ p.T
            E8 = a @ E8 @ a.T + (aFn + aFn.T) + gamma * (Mn + w8)
            M = Mn + noise8
            Gm = p @ Sk1
            F = gamma * Gm
            E[s, k + 1] = E8[:6, :6]; Em[s, k + 1] = E8[6, :7]; Eb[s, k + 1] = E8[7]
            Sk = Sk1
    return E, Em, Eb
