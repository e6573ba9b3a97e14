// collision.hip -- from a screen's pairs list to collision probabilities (include/mpcx.h: mpcx_covariance_*, mpcx_collision_probability*).
//   covariance_kernel              chains the state-transition matrices the discretiser integrates anyway (the A block of every stage
//                                  record) into a position / velocity covariance at every node of every trajectory, in m and m/s;
//   collision_probability_kernel   for every listed pair: both objects' states and position covariances at the pair's time of closest
//                                  approach, the encounter plane, and the Gaussian's integral over the combined hard-body disc in it
//                                  (the short-encounter model), by a fixed 64-point Gauss-Legendre rule.
// Both are small next to the discretisation in front of them: they are written for a fixed operation order (the numpy restatement
// tests/collision_reference.py follows it line by line), not for speed.  No atomics, nothing crosses a workgroup.
// The encounter frame, the encounter-plane covariance and the butterfly are collision_device.hpp's, shared with avoidance.hip and
// avoidance_joint.hip; the linearisation step enc_linearise (encounter_host.hpp) is defined here, for them and for the covariance.
#include "collision_device.hpp"
#include "covariance_device.hpp"
#include "encounter_host.hpp"

#include <math.h>

namespace mpcx {

// ---------------------------------------------------------------- covariance along trajectories

// tf [S] of the linearisation: tr_tf, the span in the satellite's own time unit.  A satellite without one is linearised with tf = 1
// (enc_linearise); cov_status and cp_mover make the same test and give that satellite MPCX_ST_BADK and NaN whatever the discretiser
// returns.
__global__ __launch_bounds__(256) void enc_tf_kernel(int S, const double *units, const double *span, double *tf)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= S) return;
    double v;
    tf[s] = tr_tf(span[2 * s], span[2 * s + 1], units[2 * s + 1], v) ? v : 1.0;
}

int enc_linearise(mpcx_ctx *ctx, const EncProblem &p, const LinWorkspace &ws, hipStream_t stream, bool drag_column)
{
    const int flags = p.flags | (drag_column ? MPCX_FLAG_DRAG_COLUMN : 0);
    hipLaunchKernelGGL(enc_tf_kernel, dim3((unsigned)((p.S + 255) / 256)), dim3(256), 0, stream, p.S, p.units, p.span, ws.tf);
    MPCX_HIP(ctx, hipGetLastError());
    return mpcx_discretize_stages_ragged_dev(ctx, p.S, p.K, p.Ks, p.K, p.Ks, p.Y, p.U, ws.tf, p.consts, flags, p.max_step, ws.stage, ws.dstat,
                                             stream);
}

struct CovArgs {
    int S, K;
    const int32_t *Ks;
    const double *stage, *units, *span, *P0, *q;
    const int32_t *dstat;             // the discretiser's status [S]
    double *P;
    int32_t *status;
};

// One wave per satellite; lane l < 36 owns entry (l / 6, l % 6) of the 6 x 6 matrices, the other lanes only help with the fills.
// Per node interval: Phi~ = D Phi D^-1 into LDS, T = Phi~ P, then N = T Phi~^T + q Q(h).  Entry (i, j) and entry (j, i) of N run
// the same operations on the same operands -- the sum for (min, max) -- so P is symmetric to the bit.  Sums run m = 0 .. 5 in order.
__global__ __launch_bounds__(64) void covariance_kernel(CovArgs a)
{
    __shared__ double phi[36], Pm[36], T[36];
    const int s = blockIdx.x, lane = threadIdx.x;
    const bool own = lane < 36;
    const int i = own ? lane / 6 : 0, j = own ? lane - 6 * (lane / 6) : 0;
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    const int nn = a.Ks ? a.Ks[s] : a.K;
    const double ta = a.span[2 * s], tb = a.span[2 * s + 1], Tu = a.units[2 * s + 1];
    const double qs = a.q ? a.q[s] : 0.0;
    double pij = a.P0[(size_t)s * 36 + lo * 6 + hi];                 // the upper triangle alone is read
    const int st = cov_status(nn, a.K, ta, tb, Tu, a.dstat + s, own && !cp_finite(pij));
    double *Ps = a.P + (size_t)s * a.K * 36;
    if (lane == 0) a.status[s] = st;
    if (st != MPCX_ST_OK) {
        cov_fill(Ps, lane, 0, a.K * 36, cp_nan());
        return;
    }
    cov_fill(Ps, lane, nn * 36, a.K * 36, 0.0);                      // columns past the satellite's count
    const double h = (tb - ta) / (double)(nn - 1);
    const double qQ = qs * cov_noise_entry(lo, hi, h);
    if (own) { Pm[lane] = pij; Ps[lane] = pij; }
    for (int k = 0; k + 1 < nn; ++k) {
        const double *A = a.stage + ((size_t)s * (a.K - 1) + k) * MPCX_STAGE_DOUBLES;      // 7 x 7, row-major: its upper-left 6 x 6
        if (own) {
            phi[lane] = cov_scale6(A[i * 7 + j], i, j, Tu);
        }
        __syncthreads();
        if (own) {
            double acc = phi[i * 6] * Pm[j];
#pragma unroll
            for (int m = 1; m < 6; ++m) acc = acc + phi[i * 6 + m] * Pm[m * 6 + j];
            T[lane] = acc;
        }
        __syncthreads();
        if (own) {
            double acc = T[lo * 6] * phi[hi * 6];
#pragma unroll
            for (int m = 1; m < 6; ++m) acc = acc + T[lo * 6 + m] * phi[hi * 6 + m];
            pij = acc + qQ;
            Pm[lane] = pij;
            Ps[(size_t)(k + 1) * 36 + lane] = pij;
        }
        __syncthreads();
    }
}

int cov_enqueue(mpcx_ctx *ctx, int S, int K, const int32_t *Ks, const double *stage, const int32_t *dstat, const double *units,
                const double *span, const double *P0, const double *q, double *P, int32_t *status, hipStream_t stream)
{
    const CovArgs a{S, K, Ks, stage, units, span, P0, q, dstat, P, status};
    hipLaunchKernelGGL(covariance_kernel, dim3((unsigned)S), dim3(64), 0, stream, a);
    MPCX_HIP(ctx, hipGetLastError());
    return MPCX_OK;
}

// workspace of the _dev call: [the linearisation's][zero thrust S 3 K]
struct CovWorkspace : LinWorkspace {
    double *uzero;
    size_t bytes;
    CovWorkspace(void *base, int S, int K)
    {
        Carver c(base);
        carve(c, S, K);
        uzero = c.take<double>((size_t)S * 3 * K);
        bytes = c.bytes();
    }
};

// ---------------------------------------------------------------- collision probability of listed pairs

struct CpArgs {
    int n;
    const double *pairs;
    CpSide row, col;
    double mu;
    double *out;
    int32_t *status;
};

// 1/2 [erf(b) - erf(a)] for a <= b, through erfc on the side where both are: the difference of two values near 1 keeps no digits
__device__ __forceinline__ double cp_half_erf_diff(double a, double b)
{
    if (a > 0.0) return 0.5 * (erfc(a) - erfc(b));
    if (b < 0.0) return 0.5 * (erfc(-b) - erfc(-a));
    return 0.5 * (erf(b) - erf(a));
}

// One wave per pair, lane l is quadrature node l.  The setup is the same for all 64 lanes and computed by all of them; the sum is
// an xor butterfly (every lane ends with the same bits), lane 0 stores.
__global__ __launch_bounds__(64) void collision_probability_kernel(CpArgs a)
{
    const int pr = blockIdx.x, lane = threadIdx.x;
    if (pr >= a.n) return;
    const double *row = a.pairs + (size_t)pr * 4;
    const double t = row[3];
    double o[MPCX_NPC];
#pragma unroll
    for (int c = 0; c < MPCX_NPC; ++c) o[c] = cp_nan();
    int st;
    double pa[3], va[3], Ca[6], Ra, pb[3], vb[3], Cb[6], Rb;
    st = cp_object(a.row, row[0], t, a.mu, pa, va, Ca, Ra);
    if (st == MPCX_ST_OK) st = cp_object(a.col, row[1], t, a.mu, pb, vb, Cb, Rb);
    if (st == MPCX_ST_OK) {
        double d[3], w[3], Cs[6];
#pragma unroll
        for (int c = 0; c < 3; ++c) { d[c] = pb[c] - pa[c]; w[c] = vb[c] - va[c]; }
#pragma unroll
        for (int c = 0; c < 6; ++c) Cs[c] = Ca[c] + Cb[c];
        const double R = Ra + Rb;
        double wn, mn, ew[3], e1[3], e2[3];
        CpPlane pl;
        st = cp_frame(d, w, wn, ew, mn, e1, e2);
        if (st == MPCX_ST_OK && !cp_finite(R)) st = MPCX_ST_NUMERIC;
        if (st == MPCX_ST_OK) st = cp_plane_covariance(Cs, e1, e2, pl);
        if (st == MPCX_ST_OK) {
            // the angle of the first principal axis
            const double c12 = pl.c12, df = pl.c11 - pl.c22, l1 = pl.l1, l2 = pl.l2;
            const double ph = 0.5 * atan2(2.0 * c12, df);
            const double xm = mn * cos(ph), ym = -mn * sin(ph);
            const double s1 = sqrt(l1), s2 = sqrt(l2);
            double pc = 0.0;
            if (R > 0.0) {
                const double th = 1.5707963267948966 * CP_GL[lane][0], wt = 1.5707963267948966 * CP_GL[lane][1];
                const double x = R * sin(th), cx = R * cos(th);
                const double den = 1.4142135623730951 * s2;
                const double band = cp_half_erf_diff((ym - cx) / den, (ym + cx) / den);
                const double z = (x - xm) / s1;
                double f = wt * (band * (exp(-0.5 * z * z) / (2.5066282746310002 * s1)) * cx);
                f = cp_wave_sum(f);
                pc = f < 0.0 ? 0.0 : (f > 1.0 ? 1.0 : f);
            }
            o[MPCX_PC_P] = pc; o[MPCX_PC_MISS] = mn; o[MPCX_PC_SPEED] = wn; o[MPCX_PC_SIGMA1] = s1; o[MPCX_PC_SIGMA2] = s2;
            o[MPCX_PC_MAHAL] = sqrt(xm * xm / l1 + ym * ym / l2);
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < MPCX_NPC; ++c) a.out[(size_t)pr * MPCX_NPC + c] = o[c];
        a.status[pr] = st;
    }
}

struct CpCall : EncGeometry {
    double *out;
    int32_t *status;
};
// the arguments of both entry points as a CpCall
#define MPCX_CP_CALL CpCall{MPCX_GEOMETRY(radius, cat_radius), out, status}

static int cp_check(mpcx_ctx *ctx, const CpCall &c)
{
    if (int rc = geom_check_sizes(ctx, c, "collision_probability")) return rc;
    return geom_check_arrays(ctx, c, "collision_probability", true, c.out && c.status, "pairs, Y, units, span, P, radius, out and status");
}

}  // namespace mpcx

using namespace mpcx;

extern "C" size_t mpcx_covariance_workspace_bytes(int S, int K)
{
    if (S < 1 || K < 2) return 0;
    return CovWorkspace(nullptr, S, K).bytes;
}

extern "C" int mpcx_covariance_batch_dev(mpcx_ctx *ctx, int S, int K, const int32_t *Ks, const double *X, const double *U, const double *units,
                                         const double *span, const double *consts, int flags, double max_step, const double *P0,
                                         const double *q, double *P, int32_t *status, void *workspace, void *stream)
{
    if (!ctx) return MPCX_E_BADARG;
    if (int rc = cov_check(ctx, "covariance", S, K, flags, max_step)) return rc;
    if (!X || !units || !span || !consts || !P0 || !P || !status || !workspace)
        return ctx_fail(ctx, MPCX_E_BADARG, "covariance: X, units, span, consts, P0, P, status and workspace are required");
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const CovWorkspace ws(workspace, S, K);
    if (!U) MPCX_HIP(ctx, hipMemsetAsync(ws.uzero, 0, (size_t)S * 3 * K * sizeof(double), st));
    EncProblem lin{};
    lin.S = S; lin.K = K; lin.Ks = Ks; lin.Y = X; lin.U = U ? U : ws.uzero; lin.units = units; lin.span = span; lin.consts = consts;
    lin.flags = flags; lin.max_step = max_step;
    if (int rc = enc_linearise(ctx, lin, ws, st)) return rc;
    return cov_enqueue(ctx, S, K, Ks, ws.stage, ws.dstat, units, span, P0, q, P, status, st);
}

extern "C" int mpcx_covariance_batch(mpcx_ctx *ctx, int S, int K, const int32_t *Ks, const double *X, const double *U, const double *units,
                                     const double *span, const double *consts, int flags, double max_step, const double *P0, const double *q,
                                     double *P, int32_t *status)
{
    if (!ctx) return MPCX_E_BADARG;
    if (int rc = cov_check(ctx, "covariance", S, K, flags, max_step)) return rc;
    if (!X || !units || !span || !consts || !P0 || !P || !status)
        return ctx_fail(ctx, MPCX_E_BADARG, "covariance: X, units, span, consts, P0, P and status are required");
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    DeviceArena ar(ctx);
    double *dX = ar.upload(X, (size_t)S * 7 * K), *dU = U ? ar.upload(U, (size_t)S * 3 * K) : nullptr;
    double *du = ar.upload(units, (size_t)S * 2), *dsp = ar.upload(span, (size_t)S * 2), *dc = ar.upload(consts, (size_t)S * MPCX_NCONST);
    double *dP0 = ar.upload(P0, (size_t)S * 36), *dq = q ? ar.upload(q, S) : nullptr;
    int32_t *dKs = Ks ? ar.upload(Ks, S) : nullptr;
    double *dP = ar.result(P, (size_t)S * K * 36);
    int32_t *dst = ar.result(status, (size_t)S);
    char *dws = ar.alloc<char>(mpcx_covariance_workspace_bytes(S, K));
    return host_run(ctx, ar, 0, [&](void *, hipStream_t st) {
        return mpcx_covariance_batch_dev(ctx, S, K, dKs, dX, dU, du, dsp, dc, flags, max_step, dP0, dq, dP, dst, dws, st);
    });
}

static int cp_enqueue(mpcx_ctx *ctx, const CpCall &c, hipStream_t st)
{
    CpSide row, col;
    enc_sides(c, row, col);
    const CpArgs a{c.n, c.pairs, row, col, c.mu, c.out, c.status};
    hipLaunchKernelGGL(collision_probability_kernel, dim3((unsigned)c.n), dim3(64), 0, st, a);
    MPCX_HIP(ctx, hipGetLastError());
    return MPCX_OK;
}

extern "C" int mpcx_collision_probability_dev(mpcx_ctx *ctx, int n, const double *pairs, int S, int K, const int32_t *Ks, const double *Y,
                                              const double *units, const double *span, const double *P, const double *radius, int D,
                                              int cat_K, const int32_t *cat_Ks, const double *cat_Y, const double *cat_units,
                                              const double *cat_span, const double *cat_P, const double *cat_radius, double mu, double *out,
                                              int32_t *status, void *stream)
{
    if (!ctx) return MPCX_E_BADARG;
    const CpCall c = MPCX_CP_CALL;
    if (int rc = cp_check(ctx, c)) return rc;
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    return cp_enqueue(ctx, c, (hipStream_t)stream);
}

extern "C" int mpcx_collision_probability(mpcx_ctx *ctx, int n, const double *pairs, int S, int K, const int32_t *Ks, const double *Y,
                                          const double *units, const double *span, const double *P, const double *radius, int D, int cat_K,
                                          const int32_t *cat_Ks, const double *cat_Y, const double *cat_units, const double *cat_span,
                                          const double *cat_P, const double *cat_radius, double mu, double *out, int32_t *status)
{
    if (!ctx) return MPCX_E_BADARG;
    const CpCall c = MPCX_CP_CALL;
    if (int rc = cp_check(ctx, c)) return rc;
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    DeviceArena ar(ctx);
    CpCall d = c;
    geom_upload(ar, d);
    d.out = ar.result(out, (size_t)n * MPCX_NPC);
    d.status = ar.result(status, (size_t)n);
    return host_run(ctx, ar, 0, [&](void *, hipStream_t st) { return cp_enqueue(ctx, d, st); });
}
#undef MPCX_CP_CALL
