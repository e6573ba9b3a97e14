// avoidance_window.hip -- avoidance for slow encounters: a target on the window probability (include/mpcx.h: mpcx_avoidance_window*).
//   avoidance_window_kernel   for every listed row, after collision_window_sensitivity_kernel (collision_window.hip) has left the
//                             row's Q(0) = START + ENTRIES and dQ/du: the direction of steepest descent of Q per unit of effort, its
//                             response at every node through the linearised dynamics, and the step along it that brings Q -- the
//                             window rule itself, evaluated at the shifted means, not its linearisation -- down to target_p.
// One wave per row.  The kernel is the row's bookkeeping; the direction, the response chain, Q(alpha) and the step search are
// avoidance_window_device.hpp's, which awr_solve_kernel (avoidance_window_refine.hip) runs about what was flown.  No atomics, nothing
// crosses a workgroup.  tests/avoidance_window_reference.py restates the operation order.
#include "avoidance_window_device.hpp"
#include "encounter_host.hpp"

#include <math.h>

namespace mpcx {

__global__ __launch_bounds__(64) void avoidance_window_kernel(AwArgs a)
{
    __shared__ double rec[2][CP_REC_PAD], xs[2][8];
    const int pr = blockIdx.x, lane = threadIdx.x, h = lane >> 5, ll = lane & 31;
    if (pr >= a.n) return;
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
        int ke[2];
        aw_row(a, a.pairs + (size_t)pr * 4, wo, dx, nullptr, r, ke);
        // ---- the direction, du for alpha = 1, into du
        double Gam = 0.0, dv[2] = {0.0, 0.0}, um[2] = {0.0, 0.0};
        aw_direction(a, r, g, du, lane, Gam, dv, um);
        if (!(Gam > 0.0) || !cp_finite(Gam)) st = MPCX_ST_SINGULAR;
        __syncthreads();                                             // du is read back by other lanes below
        if (st == MPCX_ST_OK) {
            aw_chain(a, r, ke, du, dx, rec, xs, h, ll);              // the unit response at the nodes 0 .. k(t_b) + 1
            // ---- the step: double from the first-order step in ln Q until Q <= target_p, then close the bracket
            const double f0 = log(Q0 / a.target);
            double lo = 0.0, flo = f0, hi = 0.0, fhi = 0.0, alpha = Q0 * f0 / Gam, Q1 = Q0;
            int evals = 0;
            bool found = false;
            while (st == MPCX_ST_OK) {                               // bracketing
                if (evals == a.max_eval) { st = MPCX_ST_INFEASIBLE; break; }
                Q1 = aw_eval<false>(a, r, alpha, lane, st);
                ++evals;
                if (st != MPCX_ST_OK) break;
                if (!(Q1 >= 0.0) || !cp_finite(Q1) || !cp_finite(alpha)) { st = MPCX_ST_NUMERIC; break; }
                const double f = log(Q1 / a.target);
                if (fabs(f) <= a.tol) { found = true; break; }
                if (f <= 0.0) { hi = alpha; fhi = f; break; }
                lo = alpha; flo = f;
                alpha = 2.0 * alpha;
            }
            aw_close<false>(a, r, lane, lo, flo, hi, fhi, found, alpha, Q1, evals, st);
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
    CpSide row, col;
    enc_sides(c, row, col);
    const AwArgs a{c.n, c.K, c.cat_Y ? 1 : 2, c.who, c.pairs, row, col, c.mu, c.panels, ws.stage, ws.dstat, c.target, c.tol,
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
    const AwCall c = MPCX_AW_CALL;
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
    const AwCall c = MPCX_AW_CALL;
    if (int rc = aw_check(ctx, c, AW_NAME)) return rc;
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    DeviceArena ar(ctx);
    AwCall d = c;
    const size_t NS = cat_Y ? 1 : 2;
    enc_upload(ar, d); d.half = ar.upload(half_window, (size_t)n);
    d.out = ar.result(out, (size_t)n * MPCX_NAW);
    d.du = ar.result(du, (size_t)n * NS * 3 * K);
    d.sens = ar.result(sens, (size_t)n * NS * 3 * K);
    d.status = ar.result(status, (size_t)n);
    return host_run(ctx, ar, mpcx_avoidance_window_workspace_bytes(n, S, K, panels),
                    [&](void *ws, hipStream_t st) { return aw_enqueue(ctx, d, ws, st); });
}
