// avoidance_window_device.hpp -- what avoidance_window_kernel (avoidance_window.hip) and awr_solve_kernel
// (avoidance_window_refine.hip) share, each written once: the solve of a row for the step along the steepest descent of its window
// probability Q, about the given plan (pass 0) or about what was flown (the refine solve).
//   the row                   AwArgs (what both kernels' arguments begin with), AwRow and aw_row (the window, the radius, the movers)
//   the direction             aw_direction: the steepest descent of Q per unit of effort for alpha = 1, Gamma, delta-v, u_max
//   the response              aw_chain: x_0 = 0, x_k+1 = A_k x_k + B_kn[k] u_k + B_kp[k] u_k+1 over the stage records
//   Q(alpha)                  aw_shift (the mean moved by the responses), aw_eval (the window rule at the moved means)
//   the step                  aw_close: the Illinois rule on f = ln Q(alpha) - ln target_p, behind the kernels' own bracketing
// PREV, the template argument of aw_shift, aw_eval and aw_close: whether the row has flown a manoeuvre before, whose response
// X_prev is taken off the mean beside alpha X_e -- the refine solve -- or not -- pass 0.
// One wave per row.  aw_chain runs the two objects of a row on the two half-waves and sends a node's A | B_kn | B_kp through LDS;
// every evaluation of Q(alpha) is collision_window_kernel's loop -- lane l time node l of the current panel, the ball term dealt
// over the lanes, xor butterflies -- with aw_shift between cw_node_at and cw_rate (collision_window.hip names the three statements
// of that loop).  The step search is wave-uniform scalar code.  No atomics, nothing crosses a workgroup, every sum has a fixed order:
// tests/avoidance_window_reference.py and tests/avoidance_window_refine_reference.py restate it.
#pragma once
#include "collision_window_device.hpp"

namespace mpcx {

// what both kernels are called with; AwrArgs (avoidance_window_refine.hip) adds the refinement's own
struct AwArgs {
    int n, K, NS, who;                // K: the constellation's row length (stage records, du, sens); NS: slots of du and sens per row
    const double *pairs;
    CpSide row, col;
    double mu;
    int panels;
    const double *stage;              // [S][K-1][MPCX_STAGE_DOUBLES]
    const int32_t *dstat;             // the discretiser's status [S]
    double target, tol;
    int max_eval;
    const double *wout;               // the sensitivity kernel's out [n][MPCX_NPW] and status [n]
    const int32_t *wstat;
    const double *g;                  // its sens [n][NS][3][K]
    double *dx;                       // workspace: the responses at the nodes, [2][K][6] each, one (pass 0) or two (refine) per row
    double *out, *du;
    int32_t *status;
};

// what an evaluation of Q(alpha) needs of the row (wave-uniform)
struct AwMover {
    bool moves;
    CpMover mv;
    double Tu;
};
struct AwRow {
    double fi, fj, ta, hp, R;
    AwMover m0, m1;                   // slot 0 (object i), slot 1 (object j); two members, not an array: a selection, never an address
    const double *xe, *xp;            // the responses to the direction and (PREV) to the manoeuvre flown before, [2][K][6] each
    size_t K;
    __device__ __forceinline__ const AwMover &slot(int sl) const { return sl ? m1 : m0; }
    __device__ __forceinline__ AwMover &slot(int sl) { return sl ? m1 : m0; }
};

// The row `row` of the list whose window call left `wo`: its window in panels, both objects at t (the radius, the movers) and at the
// window's end (ke: the last interval the chain has to reach, per object).  The sensitivity kernel passed these tests: the
// statuses are OK.
__device__ __forceinline__ void aw_row(const AwArgs &a, const double *row, const double *wo, const double *xe, const double *xp, AwRow &r,
                                       int (&ke)[2])
{
    const double t = row[3];
    r.fi = row[0]; r.fj = row[1]; r.ta = wo[MPCX_PW_TA]; r.hp = (wo[MPCX_PW_TB] - wo[MPCX_PW_TA]) / (double)a.panels;
    r.m0.moves = a.who != 1; r.m1.moves = a.NS == 2 && a.who != 0;
    r.xe = xe; r.xp = xp; r.K = (size_t)a.K;
    CpNode n0[2], ne[2];
    {
        double p[3], v[3];
        cp_state(a.row, r.fi, t, p, v, n0[0]);
        cp_state(a.col, r.fj, t, p, v, n0[1]);
        cp_state(a.row, r.fi, wo[MPCX_PW_TB], p, v, ne[0]);
        cp_state(a.col, r.fj, wo[MPCX_PW_TB], p, v, ne[1]);
    }
    ke[0] = ne[0].k; ke[1] = ne[1].k;
    r.R = a.row.radius[n0[0].o] + a.col.radius[n0[1].o];
#pragma unroll
    for (int sl = 0; sl < 2; ++sl) {
        r.slot(sl).mv = CpMover{};
        r.slot(sl).Tu = 1.0;
        if (!r.slot(sl).moves) continue;
        cp_mover(a.row, a.dstat, n0[sl], r.K, r.slot(sl).mv);
        r.slot(sl).Tu = a.row.units[2 * r.slot(sl).mv.o + 1];
    }
}

// The direction: steepest descent of Q per unit of effort from the sensitivities g, du for alpha = 1 into e [NS][3][K] (zero past a
// mover's nodes and in the slot of an object that does not move); added to the caller's zeros: Gamma, and per slot that moves the
// delta-v and the largest |du_m| for alpha = 1.  Called by the whole wave; e is read back by other lanes only behind the caller's
// barrier.
__device__ __forceinline__ void aw_direction(const AwArgs &a, const AwRow &r, const double *g, double *e, int lane, double &Gam,
                                             double (&dv)[2], double (&um)[2])
{
    const size_t K = r.K;
#pragma unroll
    for (int sl = 0; sl < 2; ++sl) {
        if (sl >= a.NS) continue;
        const int nn = r.slot(sl).moves ? r.slot(sl).mv.nn : 0;
        for (int c = 0; c < 3; ++c)
            for (int m = nn + lane; m < a.K; m += 64) e[((size_t)sl * 3 + c) * K + m] = 0.0;
        if (!r.slot(sl).moves) continue;
        double sG = 0.0, sdv = 0.0, sum = 0.0;
        for (int m = lane; m < nn; m += 64) {
            const double cm = r.slot(sl).mv.cfac / r.slot(sl).mv.mass[m];
            const double wm = (m == 0 || m == nn - 1) ? 0.5 * r.slot(sl).mv.hn : r.slot(sl).mv.hn;
            double gh[3], da[3], dn[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                gh[c] = g[((size_t)sl * 3 + c) * K + m] / cm;
                da[c] = -gh[c] / wm;
                dn[c] = da[c] / cm;
                e[((size_t)sl * 3 + c) * K + m] = dn[c];
            }
            sG = sG + (gh[0] * gh[0] + gh[1] * gh[1] + gh[2] * gh[2]) / wm;
            sdv = sdv + wm * sqrt(da[0] * da[0] + da[1] * da[1] + da[2] * da[2]);
            sum = fmax(sum, sqrt(dn[0] * dn[0] + dn[1] * dn[1] + dn[2] * dn[2]));
        }
        Gam = Gam + cp_wave_sum(sG);
        dv[sl] = cp_wave_sum(sdv); um[sl] = cp_wave_max(sum);
    }
}

// The response x_0 = 0, x_k+1 = A_k x_k + B_kn[k] u_k + B_kp[k] u_k+1 of the movers to u [NS][3][K] at the nodes 0 .. ke + 1 into
// x [2][K][6]: half h of the wave runs the object of slot h, lanes 0..6 of a half own the entries of x_k.  Called by the whole
// block; ends behind a barrier.
__device__ __forceinline__ void aw_chain(const AwArgs &a, const AwRow &r, const int (&ke)[2], const double *u, double *x,
                                         double (&rec)[2][CP_REC_PAD], double (&xs)[2][8], int h, int ll)
{
    const size_t K = r.K;
    const bool mine = h < a.NS && r.slot(h).moves;
    const int kme = h ? ke[1] : ke[0];
    const int kmax = r.m0.moves ? (r.m1.moves && ke[1] > ke[0] ? ke[1] : ke[0]) : ke[1];
    const double *srec = a.stage + (size_t)(h ? r.m1.mv.o : r.m0.mv.o) * (K - 1) * MPCX_STAGE_DOUBLES;     // (read only where `mine`)
    const double *uh = u + (size_t)h * 3 * K;
    double *xh = x + (size_t)h * K * 6;
    if (mine && ll < 7) {
        xs[h][ll] = 0.0;
        if (ll < 6) xh[ll] = 0.0;
    }
    for (int q = 0; q <= kmax; ++q) {
        const bool act = mine && q <= kme;
        if (act) {
            const double *rp = srec + (size_t)q * MPCX_STAGE_DOUBLES;
            rec[h][ll] = rp[ll]; rec[h][ll + 32] = rp[ll + 32];
            if (ll + 64 < CP_REC) rec[h][ll + 64] = rp[ll + 64];
        }
        __syncthreads();
        double xn = 0.0;
        if (act && ll < 7) {
            xn = rec[h][ll * 7] * xs[h][0];
#pragma unroll
            for (int c = 1; c < 7; ++c) xn = xn + rec[h][ll * 7 + c] * xs[h][c];
#pragma unroll
            for (int c = 0; c < 3; ++c) xn = xn + rec[h][49 + ll * 3 + c] * uh[(size_t)c * K + q];
#pragma unroll
            for (int c = 0; c < 3; ++c) xn = xn + rec[h][70 + ll * 3 + c] * uh[(size_t)c * K + q + 1];
        }
        __syncthreads();
        if (act && ll < 7) {
            xs[h][ll] = xn;
            if (ll < 6) xh[(size_t)(q + 1) * 6 + ll] = xn;
        }
    }
    __syncthreads();                                                 // x is read back by other lanes
}

// entry c of a basis b on the two node states x0, x1 that bracket a time
__device__ __forceinline__ double aw_on_nodes(const double (&b)[4], const double *x0, const double *x1, int c)
{
    return b[0] * x0[c] + b[1] * x0[3 + c] + b[2] * x1[c] + b[3] * x1[3 + c];
}

// The mean relative state at the time the two objects were placed at nq, moved by sgn alpha X_e, or (PREV) by sgn (alpha X_e -
// X_prev).  The two sums are written as they always were: the build contracts a multiply-add inside one expression.
template <bool PREV>
__device__ __forceinline__ void aw_shift(const AwRow &r, const CpNode (&nq)[2], double alpha, CwNode &nd)
{
    double de[3] = {0.0, 0.0, 0.0}, we[3] = {0.0, 0.0, 0.0}, dp[3] = {0.0, 0.0, 0.0}, wp[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int sl = 0; sl < 2; ++sl) {
        if (!r.slot(sl).moves) continue;
        CwBasis b;
        cw_basis(nq[sl], r.slot(sl).mv.L, r.slot(sl).Tu, r.slot(sl).mv.htau, b);
        const double sgn = sl ? 1.0 : -1.0;
        const size_t at = ((size_t)sl * r.K + nq[sl].k) * 6;
        const double *e0 = r.xe + at, *e1 = e0 + 6;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            de[c] = de[c] + sgn * aw_on_nodes(b.p, e0, e1, c);
            we[c] = we[c] + sgn * aw_on_nodes(b.v, e0, e1, c);
        }
        if constexpr (PREV) {
            const double *p0 = r.xp + at, *p1 = p0 + 6;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                dp[c] = dp[c] + sgn * aw_on_nodes(b.p, p0, p1, c);
                wp[c] = wp[c] + sgn * aw_on_nodes(b.v, p0, p1, c);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if constexpr (PREV) { nd.d[c] = nd.d[c] + (alpha * de[c] - dp[c]); nd.w[c] = nd.w[c] + (alpha * we[c] - wp[c]); }
        else { nd.d[c] = nd.d[c] + alpha * de[c]; nd.w[c] = nd.w[c] + alpha * we[c]; }
    }
}

// Q(alpha) = START + ENTRIES of the window rule at the moved means: the row's covariances, frames (the pole of the unmoved w) and
// rules.  Called by the whole wave; the same bits on every lane.  st: MPCX_ST_NUMERIC for a node that fails.
template <bool PREV>
__device__ __forceinline__ double aw_eval(const AwArgs &a, const AwRow &r, double alpha, int lane, int &st)
{
    double entries = 0.0;
    CwNode nd;
    CpNode nq[2];
    for (int p = 0; p < a.panels; ++p) {
        const double tau = (r.ta + (double)p * r.hp) + (0.5 * r.hp) * (1.0 + CP_GL[lane][0]);
        const int sl = cw_node_at(a.row, a.col, r.fi, r.fj, tau, a.mu, nd, nq[0], nq[1]);
        if (__any(sl != MPCX_ST_OK)) { st = MPCX_ST_NUMERIC; return cp_nan(); }
        aw_shift<PREV>(r, nq, alpha, nd);
        const double rate = cw_rate(nd, r.R);
        entries = entries + cp_wave_sum(((0.5 * r.hp) * CP_GL[lane][1]) * rate);
    }
    if (cw_node_at(a.row, a.col, r.fi, r.fj, r.ta, a.mu, nd, nq[0], nq[1]) != MPCX_ST_OK) { st = MPCX_ST_NUMERIC; return cp_nan(); }
    aw_shift<PREV>(r, nq, alpha, nd);
    const double start = nd.cden * cp_wave_sum(cw_ball_share(nd, r.R, lane));
    return start + entries;
}

// The closing of a bracket lo < hi on the root of f = ln Q(alpha) - ln target_p (flo = f(lo) > 0 >= fhi = f(hi)) by the Illinois
// rule: the secant of the bracket's ends; the end kept twice running has its f halved; a secant point that is not strictly inside
// the bracket is replaced by the middle.  The bracketing before it is the kernels' own: pass 0 knows f(0) > 0 and only doubles, the
// refine solve doubles or halves.  Nothing is done when the bracketing ended with a status or `found` alpha already.  evals counts
// the evaluations of both phases: MPCX_ST_MAXITER when max_eval are used up here.  Ends with the accepted alpha and Q1 = Q(alpha),
// |f| <= tol, or with a status.
template <bool PREV>
__device__ __forceinline__ void aw_close(const AwArgs &a, const AwRow &r, int lane, double lo, double flo, double hi, double fhi, bool found,
                                         double &alpha, double &Q1, int &evals, int &st)
{
    int side = 0;
    while (st == MPCX_ST_OK && !found) {
        if (evals == a.max_eval) { st = MPCX_ST_MAXITER; break; }
        alpha = lo + (hi - lo) * (flo / (flo - fhi));
        if (!(alpha > lo && alpha < hi)) alpha = 0.5 * (lo + hi);
        Q1 = aw_eval<PREV>(a, r, alpha, lane, st);
        ++evals;
        if (st != MPCX_ST_OK) break;
        if (!(Q1 >= 0.0) || !cp_finite(Q1)) { st = MPCX_ST_NUMERIC; break; }
        const double f = log(Q1 / a.target);
        if (fabs(f) <= a.tol) { found = true; break; }
        if (f > 0.0) {
            lo = alpha; flo = f;
            if (side == 1) fhi = 0.5 * fhi;
            side = 1;
        } else {
            hi = alpha; fhi = f;
            if (side == -1) flo = 0.5 * flo;
            side = -1;
        }
    }
}

}  // namespace mpcx
