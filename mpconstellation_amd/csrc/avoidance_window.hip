// avoidance_window.hip -- avoidance for slow encounters: a target on the window probability (include/mpcx.h: mpcx_avoidance_window*).
//   avoidance_window_kernel   for every listed row, after collision_window_sensitivity_kernel (collision_window.hip) has left the
//                             row's Q(0) = START + ENTRIES and dQ/du: the direction of steepest descent of Q per unit of effort, its
//                             response at every node through the linearised dynamics, and the step along it that brings Q -- the
//                             window rule itself, evaluated at the shifted means, not its linearisation -- down to target_p.
// One wave per row.  The response is a forward chain of 7 x 7 products: the two half-waves run the two objects of a row side by side,
// lanes 0..6 of a half own the entries of dx_k, a node's A | B_kn | B_kp goes through LDS.  Every evaluation of Q(alpha) is
// collision_window_kernel's loop -- lane l time node l of the current panel, cw_node, cw_rate, the ball term dealt over the lanes,
// xor butterflies -- with the mean moved by alpha (dd, dw) between cw_node and cw_rate.  The step-length search is wave-uniform
// scalar code.  No atomics, nothing crosses a workgroup.  tests/avoidance_window_reference.py restates the operation order.
#include "collision_window_device.hpp"
#include "encounter_host.hpp"

#include <math.h>

namespace mpcx {

struct AwArgs {
    int n, K, NS, who;                // K: the constellation's row length (stage records, du, sens); NS: slots of du and sens per row
    const double *pairs;
    CpSide row, col;
    double mu;
    const double *half;
    int panels;
    const double *stage;              // [S][K-1][MPCX_STAGE_DOUBLES]
    const int32_t *dstat;             // the discretiser's status [S]
    double target, tol;
    int max_eval;
    const double *wout;               // the sensitivity kernel's out [n][MPCX_NPW] and status [n]
    const int32_t *wstat;
    const double *g;                  // its sens [n][NS][3][K]
    double *dx;                       // workspace: the unit response at the nodes [n][2][K][6]
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
    const double *dx;                 // [2][K][6]
    size_t K;
    __device__ __forceinline__ const AwMover &slot(int sl) const { return sl ? m1 : m0; }
    __device__ __forceinline__ AwMover &slot(int sl) { return sl ? m1 : m0; }
};

// alpha times the response of the mean relative state at the time the two objects were placed at nq: added to nd.d, nd.w
__device__ __forceinline__ void aw_shift(const AwRow &r, const CpNode (&nq)[2], double alpha, CwNode &nd)
{
    double dd[3] = {0.0, 0.0, 0.0}, dw[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int sl = 0; sl < 2; ++sl) {
        if (!r.slot(sl).moves) continue;
        CwBasis b;
        cw_basis(nq[sl], r.slot(sl).mv.L, r.slot(sl).Tu, r.slot(sl).mv.htau, b);
        const double sgn = sl ? 1.0 : -1.0;
        const double *x0 = r.dx + ((size_t)sl * r.K + nq[sl].k) * 6, *x1 = x0 + 6;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            dd[c] = dd[c] + sgn * (b.p[0] * x0[c] + b.p[1] * x0[3 + c] + b.p[2] * x1[c] + b.p[3] * x1[3 + c]);
            dw[c] = dw[c] + sgn * (b.v[0] * x0[c] + b.v[1] * x0[3 + c] + b.v[2] * x1[c] + b.v[3] * x1[3 + c]);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) { nd.d[c] = nd.d[c] + alpha * dd[c]; nd.w[c] = nd.w[c] + alpha * dw[c]; }
}

// Q(alpha) = START + ENTRIES of the window rule at the means (d + alpha dd, w + alpha dw): the row's covariances, frames (the pole of
// the unmoved w) and rules.  Called by the whole wave; the same bits on every lane.  st: MPCX_ST_NUMERIC for a node that fails.
__device__ __forceinline__ double aw_eval(const AwArgs &a, const AwRow &r, double alpha, int lane, int &st)
{
    double entries = 0.0;
    CwNode nd;
    CpNode nq[2];
    for (int p = 0; p < a.panels; ++p) {
        const double tau = (r.ta + (double)p * r.hp) + (0.5 * r.hp) * (1.0 + CP_GL[lane][0]);
        const int sl = cw_node_at(a.row, a.col, r.fi, r.fj, tau, a.mu, nd, nq[0], nq[1]);
        if (__any(sl != MPCX_ST_OK)) { st = MPCX_ST_NUMERIC; return cp_nan(); }
        aw_shift(r, nq, alpha, nd);
        const double rate = cw_rate(nd, r.R);
        entries = entries + cp_wave_sum(((0.5 * r.hp) * CP_GL[lane][1]) * rate);
    }
    if (cw_node_at(a.row, a.col, r.fi, r.fj, r.ta, a.mu, nd, nq[0], nq[1]) != MPCX_ST_OK) { st = MPCX_ST_NUMERIC; return cp_nan(); }
    aw_shift(r, nq, alpha, nd);
    const double start = nd.cden * cp_wave_sum(cw_ball_share(nd, r.R, lane));
    return start + entries;
}

__global__ __launch_bounds__(64) void avoidance_window_kernel(AwArgs a)
{
    __shared__ double rec[2][CP_REC_PAD], xs[2][8];
    const int pr = blockIdx.x, lane = threadIdx.x, h = lane >> 5, ll = lane & 31;
    if (pr >= a.n) return;
    const double *row = a.pairs + (size_t)pr * 4;
    const double t = row[3];
    const size_t K = (size_t)a.K;
    const double *g = a.g + (size_t)pr * a.NS * 3 * K, *wo = a.wout + (size_t)pr * MPCX_NPW;
    double *du = a.du + (size_t)pr * a.NS * 3 * K, *dx = a.dx + (size_t)pr * 2 * K * 6;
    double o[MPCX_NAW];
#pragma unroll
    for (int c = 0; c < MPCX_NAW; ++c) o[c] = cp_nan();
    int st = a.wstat[pr];
    const double Q0 = wo[MPCX_PW_START] + wo[MPCX_PW_ENTRIES];           // the window call's unclamped sum, its bits
    bool zero = false;
    if (st == MPCX_ST_OK && Q0 <= a.target) {
        // ---- at or below the target already (a row without a sphere is): no change
        zero = true;
        o[MPCX_AW_P0] = Q0; o[MPCX_AW_P1] = Q0; o[MPCX_AW_ALPHA] = 0.0; o[MPCX_AW_DQ_LINEAR] = 0.0;
        o[MPCX_AW_DV_I] = 0.0; o[MPCX_AW_DV_J] = 0.0; o[MPCX_AW_UMAX_I] = 0.0; o[MPCX_AW_UMAX_J] = 0.0; o[MPCX_AW_EVALS] = 0.0;
    } else if (st == MPCX_ST_OK) {
        AwRow r;
        r.fi = row[0]; r.fj = row[1]; r.ta = wo[MPCX_PW_TA]; r.hp = (wo[MPCX_PW_TB] - wo[MPCX_PW_TA]) / (double)a.panels;
        r.m0.moves = a.who != 1; r.m1.moves = a.NS == 2 && a.who != 0;
        r.dx = dx; r.K = K;
        // both objects at t and at the window's end (the sensitivity kernel passed these tests: the statuses are OK)
        CpNode n0[2], ne[2];
        {
            double p[3], v[3];
            cp_state(a.row, r.fi, t, p, v, n0[0]);
            cp_state(a.col, r.fj, t, p, v, n0[1]);
            cp_state(a.row, r.fi, wo[MPCX_PW_TB], p, v, ne[0]);
            cp_state(a.col, r.fj, wo[MPCX_PW_TB], p, v, ne[1]);
        }
        r.R = a.row.radius[n0[0].o] + a.col.radius[n0[1].o];
#pragma unroll
        for (int sl = 0; sl < 2; ++sl) {
            r.slot(sl).mv = CpMover{};
            r.slot(sl).Tu = 1.0;
            if (!r.slot(sl).moves) continue;
            cp_mover(a.row, a.dstat, n0[sl], K, r.slot(sl).mv);
            r.slot(sl).Tu = a.row.units[2 * r.slot(sl).mv.o + 1];
        }
        // ---- the direction: steepest descent of Q per unit of effort, du for alpha = 1 into du; Gamma
        double Gam = 0.0, dv[2] = {0.0, 0.0}, um[2] = {0.0, 0.0};
#pragma unroll
        for (int sl = 0; sl < 2; ++sl) {
            if (sl >= a.NS) continue;
            const int nn = r.slot(sl).moves ? r.slot(sl).mv.nn : 0;
            for (int c = 0; c < 3; ++c)
                for (int m = nn + lane; m < a.K; m += 64) du[((size_t)sl * 3 + c) * K + m] = 0.0;
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
                    du[((size_t)sl * 3 + c) * K + m] = dn[c];
                }
                sG = sG + (gh[0] * gh[0] + gh[1] * gh[1] + gh[2] * gh[2]) / wm;
                sdv = sdv + wm * sqrt(da[0] * da[0] + da[1] * da[1] + da[2] * da[2]);
                sum = fmax(sum, sqrt(dn[0] * dn[0] + dn[1] * dn[1] + dn[2] * dn[2]));
            }
            Gam = Gam + cp_wave_sum(sG);
            dv[sl] = cp_wave_sum(sdv); um[sl] = cp_wave_max(sum);
        }
        if (!(Gam > 0.0) || !cp_finite(Gam)) st = MPCX_ST_SINGULAR;
        __syncthreads();                                             // du is read back by other lanes below
        if (st == MPCX_ST_OK) {
            // ---- the unit response at the nodes 0 .. k(t_b) + 1: dx_0 = 0, dx_k+1 = A_k dx_k + B_kn[k] du_k + B_kp[k] du_k+1
            const bool mine = h < a.NS && r.slot(h).moves;
            const int kme = h ? ne[1].k : ne[0].k;
            const int kmax = r.m0.moves ? (r.m1.moves && ne[1].k > ne[0].k ? ne[1].k : ne[0].k) : ne[1].k;
            const double *srec = a.stage + (size_t)(h ? r.m1.mv.o : r.m0.mv.o) * (K - 1) * MPCX_STAGE_DOUBLES;     // (read only where `mine`)
            const double *uh = du + (size_t)h * 3 * K;
            double *xh = dx + (size_t)h * K * 6;
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
                    for (int x = 1; x < 7; ++x) xn = xn + rec[h][ll * 7 + x] * xs[h][x];
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
            __syncthreads();                                         // dx is read back by other lanes below

            // ---- the step: double from the first-order step in ln Q until Q <= target_p, then close the bracket on f = ln Q -
            // ln target_p by the Illinois rule (the secant of the bracket's ends; the end kept twice running has its f halved; a
            // secant point that is not strictly inside the bracket is replaced by the middle)
            const double f0 = log(Q0 / a.target);
            double lo = 0.0, flo = f0, hi = 0.0, fhi = 0.0, alpha = Q0 * f0 / Gam, Q1 = Q0;
            int evals = 0;
            bool found = false;
            while (st == MPCX_ST_OK) {                               // bracketing
                if (evals == a.max_eval) { st = MPCX_ST_INFEASIBLE; break; }
                Q1 = aw_eval(a, r, alpha, lane, st);
                ++evals;
                if (st != MPCX_ST_OK) break;
                if (!(Q1 >= 0.0) || !cp_finite(Q1) || !cp_finite(alpha)) { st = MPCX_ST_NUMERIC; break; }
                const double f = log(Q1 / a.target);
                if (fabs(f) <= a.tol) { found = true; break; }
                if (f <= 0.0) { hi = alpha; fhi = f; break; }
                lo = alpha; flo = f;
                alpha = 2.0 * alpha;
            }
            int side = 0;
            while (st == MPCX_ST_OK && !found) {                     // closing
                if (evals == a.max_eval) { st = MPCX_ST_MAXITER; break; }
                alpha = lo + (hi - lo) * (flo / (flo - fhi));
                if (!(alpha > lo && alpha < hi)) alpha = 0.5 * (lo + hi);
                Q1 = aw_eval(a, r, alpha, lane, st);
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
            if (st == MPCX_ST_OK) {
#pragma unroll
                for (int sl = 0; sl < 2; ++sl) {
                    if (sl >= a.NS || !r.slot(sl).moves) continue;
                    for (int c = 0; c < 3; ++c)
                        for (int m = lane; m < r.slot(sl).mv.nn; m += 64) du[((size_t)sl * 3 + c) * K + m] = alpha * du[((size_t)sl * 3 + c) * K + m];
                }
                o[MPCX_AW_P0] = Q0; o[MPCX_AW_P1] = Q1; o[MPCX_AW_ALPHA] = alpha; o[MPCX_AW_DQ_LINEAR] = -(alpha * Gam);
                o[MPCX_AW_DV_I] = alpha * dv[0]; o[MPCX_AW_DV_J] = alpha * dv[1];
                o[MPCX_AW_UMAX_I] = alpha * um[0]; o[MPCX_AW_UMAX_J] = alpha * um[1];
                o[MPCX_AW_EVALS] = (double)evals;
            }
        }
    }
    if (st != MPCX_ST_OK || zero) {                                  // a failed row is NaN throughout; one below the target: zero
        const double f = zero ? 0.0 : cp_nan();
        for (size_t e = lane; e < (size_t)a.NS * 3 * K; e += 64) du[e] = f;
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < MPCX_NAW; ++c) a.out[(size_t)pr * MPCX_NAW + c] = o[c];
        a.status[pr] = st;
    }
}

// workspace of the _dev call: [the sensitivity's][the window call's out n NPW][its status n][sens n 2 3 K][dx n 2 K 6]
struct AwWorkspace : CwsWorkspace {
    double *wout, *g, *dx;
    int32_t *wstat;
    size_t bytes;
    AwWorkspace(void *base, int n, int S, int K)
    {
        Carver c(base);
        carve_cws(c, n, S, K);
        wout = c.take<double>((size_t)n * MPCX_NPW);
        wstat = c.take<int32_t>((size_t)n);
        g = c.take<double>((size_t)n * 2 * 3 * K);
        dx = c.take<double>((size_t)n * 2 * K * 6);
        bytes = c.bytes();
    }
};

static const char *const AW_NAME = "avoidance_window";

int aw_check(mpcx_ctx *ctx, const AwCall &c, const char *name)
{
    if (int rc = cws_check(ctx, c, name, c.out && c.du && c.status, "P, radius, half_window, out, du and status")) return rc;
    if (!(c.target > 0.0 && c.target < 1.0)) return enc_fail(ctx, name, "target_p must lie strictly between 0 and 1");
    if (!(c.tol > 0.0) || !(c.tol < __builtin_inf())) return enc_fail(ctx, name, "tol must be a positive finite number");
    if (c.max_eval < 1) return enc_fail(ctx, name, "max_eval must be >= 1");
    return MPCX_OK;
}

// c.out / c.status are the manoeuvre's; the sensitivity kernel's own go to the workspace
int aw_enqueue(mpcx_ctx *ctx, const AwCall &c, void *workspace, hipStream_t st)
{
    const AwWorkspace ws(workspace, c.n, c.S, c.K);
    if (int rc = enc_linearise(ctx, c, ws, st)) return rc;
    CwsCall s = c;
    s.out = ws.wout; s.status = ws.wstat; s.state_grad = nullptr;
    s.sens = c.sens ? c.sens : ws.g;
    if (int rc = cws_enqueue(ctx, s, ws, st)) return rc;
    const CpSide row{c.S, c.K, c.Ks, c.Y, c.units, c.span, c.P, c.radius};
    const CpSide col = c.cat_Y ? CpSide{c.D, c.cat_K, c.cat_Ks, c.cat_Y, c.cat_units, c.cat_span, c.cat_P, c.cat_radius} : row;
    const AwArgs a{c.n, c.K, c.cat_Y ? 1 : 2, c.who, c.pairs, row, col, c.mu, c.half, c.panels, ws.stage, ws.dstat, c.target, c.tol,
                   c.max_eval, ws.wout, ws.wstat, s.sens, ws.dx, c.out, c.du, c.status};
    hipLaunchKernelGGL(avoidance_window_kernel, dim3((unsigned)c.n), dim3(64), 0, st, a);
    MPCX_HIP(ctx, hipGetLastError());
    return MPCX_OK;
}

}  // namespace mpcx

using namespace mpcx;

extern "C" size_t mpcx_avoidance_window_workspace_bytes(int n, int S, int K, int panels)
{
    if (n < 1 || S < 1 || K < 2 || panels < 1 || panels > MPCX_PW_MAX_PANELS) return 0;
    return AwWorkspace(nullptr, n, S, K).bytes;
}

extern "C" int mpcx_avoidance_window_dev(mpcx_ctx *ctx, int n, const double *pairs, int S, int K, const int32_t *Ks, const double *Y,
                                         const double *U, const double *units, const double *span, const double *consts, int flags,
                                         double max_step, const double *P, const double *radius, int D, int cat_K, const int32_t *cat_Ks,
                                         const double *cat_Y, const double *cat_units, const double *cat_span, const double *cat_P,
                                         const double *cat_radius, double mu, const double *half_window, int panels, int who,
                                         double target_p, double tol, int max_eval, double *out, double *du, double *sens,
                                         int32_t *status, void *workspace, void *stream)
{
    if (!ctx) return MPCX_E_BADARG;
    const AwCall c{{{n, pairs, S, K, Ks, Y, U, units, span, consts, flags, max_step, P, D, cat_K, cat_Ks, cat_Y, cat_units, cat_span, cat_P,
                     mu, target_p}, radius, cat_radius, half_window, panels, who, out, sens, nullptr, status}, tol, max_eval, du};
    if (int rc = aw_check(ctx, c, AW_NAME)) return rc;
    if (!workspace)
        return enc_fail(ctx, AW_NAME, "a workspace of mpcx_avoidance_window_workspace_bytes(n, S, K, panels) bytes is required");
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    return aw_enqueue(ctx, c, workspace, (hipStream_t)stream);
}

extern "C" int mpcx_avoidance_window(mpcx_ctx *ctx, int n, const double *pairs, int S, int K, const int32_t *Ks, const double *Y,
                                     const double *U, const double *units, const double *span, const double *consts, int flags,
                                     double max_step, const double *P, const double *radius, int D, int cat_K, const int32_t *cat_Ks,
                                     const double *cat_Y, const double *cat_units, const double *cat_span, const double *cat_P,
                                     const double *cat_radius, double mu, const double *half_window, int panels, int who, double target_p,
                                     double tol, int max_eval, double *out, double *du, double *sens, int32_t *status)
{
    if (!ctx) return MPCX_E_BADARG;
    const AwCall c{{{n, pairs, S, K, Ks, Y, U, units, span, consts, flags, max_step, P, D, cat_K, cat_Ks, cat_Y, cat_units, cat_span, cat_P,
                     mu, target_p}, radius, cat_radius, half_window, panels, who, out, sens, nullptr, status}, tol, max_eval, du};
    if (int rc = aw_check(ctx, c, AW_NAME)) return rc;
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    DeviceArena ar(ctx);
    AwCall d = c;
    const size_t NS = cat_Y ? 1 : 2;
    cws_upload(ar, d);
    d.out = ar.alloc<double>((size_t)n * MPCX_NAW);
    d.du = ar.alloc<double>((size_t)n * NS * 3 * K);
    d.sens = sens ? ar.alloc<double>((size_t)n * NS * 3 * K) : nullptr;
    d.status = ar.alloc<int32_t>(n);
    if (ar.failed()) return ar.code();
    void *ws = ctx_workspace(ctx, mpcx_avoidance_window_workspace_bytes(n, S, K, panels));
    if (!ws) return MPCX_E_NOMEM;
    if (int rc = aw_enqueue(ctx, d, ws, ctx->stream)) return rc;
    ar.download(out, d.out, (size_t)n * MPCX_NAW);
    ar.download(du, d.du, (size_t)n * NS * 3 * K);
    if (sens) ar.download(sens, d.sens, (size_t)n * NS * 3 * K);
    ar.download(status, d.status, n);
    return ar.finish();
}
