// encounter_window.hip -- the time window of every listed encounter (include/mpcx.h: mpcx_encounter_window*): for every listed row
// (i, j, ., t) the connected stretch of time about t outside which the pair's mean separation is more than nsigma combined sigmas
// (plus the summed radii) away from a collision -- the half_window that the window calls of collision_window.hip, avoidance_window.hip
// and collision_mc.hip take, chosen by one rule whether the pair closes at km/s or does not move at all.
//   encounter_window_kernel   one wave per row.  A time tau is LIVE when g(tau) = |L^-1 d| - max(R, 0) |L^-1|_F - nsigma <= 0, d and
//                             L^-1 from cw_node (collision_window_device.hpp) as it stands: no second way of forming a node.  The side
//                             before t, then the side after it: `levels` times the bracket [a, b] of offsets from t is cut into 64
//                             cells, lane l tests the end of cell l, and the first cell whose end is not live (a ballot, a
//                             find-first-set) is the next bracket.  1 + 2 levels node evaluations per lane; the two sides run one after
//                             the other so that one CwNode is alive at a time.  Lane 0 stores.  No LDS, no atomics, nothing crosses a
//                             workgroup; every row is computed from its own arguments alone, so results do not depend on the list's
//                             order, its length or the launch.
// Written for a fixed operation order (tests/encounter_window_reference.py follows it line by line).
#include "collision_window_device.hpp"
#include "encounter_host.hpp"

#include <math.h>

namespace mpcx {

struct EwArgs {
    int n;
    const double *pairs;
    CpSide row, col;
    double mu;
    const double *max_half;
    double nsigma;
    int levels;
    double *out;
    int32_t *flags, *status;
};

// g at the time tau: cw_node's status, and where that is MPCX_ST_OK
//   g = |L^-1 d| - Rp |L^-1|_F - nsigma,   |L^-1|_F over i00, i10, i11, i20, i21, i22 in that order.
// |L^-1|_F >= |L^-1|_2, so g > 0 puts every point of the sphere of radius Rp more than nsigma whitened units from the mean.
__device__ __forceinline__ int ew_g(const CpSide &row, const CpSide &col, double fi, double fj, double tau, double mu, double Rp, double nsigma,
                                    double &g)
{
    CwNode nd;
    const int st = cw_node(row, col, fi, fj, tau, mu, nd);
    if (st != MPCX_ST_OK) return st;
    const double z0 = nd.i00 * nd.d[0];
    const double z1 = nd.i10 * nd.d[0] + nd.i11 * nd.d[1];
    const double z2 = nd.i20 * nd.d[0] + nd.i21 * nd.d[1] + nd.i22 * nd.d[2];
    const double zn = sqrt(z0 * z0 + z1 * z1 + z2 * z2);
    const double fn = sqrt(nd.i00 * nd.i00 + nd.i10 * nd.i10 + nd.i11 * nd.i11 + nd.i20 * nd.i20 + nd.i21 * nd.i21 + nd.i22 * nd.i22);
    g = (zn - Rp * fn) - nsigma;
    return MPCX_ST_OK;
}

__global__ __launch_bounds__(64) void encounter_window_kernel(EwArgs a)
{
    const int pr = blockIdx.x, lane = threadIdx.x;
    if (pr >= a.n) return;
    const double *row = a.pairs + (size_t)pr * 4;
    const double fi = row[0], fj = row[1], t = row[3], H = a.max_half[pr];
    double o[MPCX_NEW];
#pragma unroll
    for (int c = 0; c < MPCX_NEW; ++c) o[c] = cp_nan();
    int fl = 0;
    // the row's own tests (wave-uniform) in the order of their statuses, as cw_row: both objects at t, max_half, the radius, the node at t
    double lo = 0.0, hi = 0.0, R = 0.0, g0 = 0.0;
    int st;
    {
        double p[3], v[3];
        CpNode na, nb;
        st = cp_state(a.row, fi, t, p, v, na);
        if (st == MPCX_ST_OK) st = cp_state(a.col, fj, t, p, v, nb);
        if (st == MPCX_ST_OK && !(H > 0.0 && cp_finite(H))) st = MPCX_ST_BADK;
        if (st == MPCX_ST_OK) {
            lo = fmax(a.row.span[2 * na.o], a.col.span[2 * nb.o]);
            hi = fmin(a.row.span[2 * na.o + 1], a.col.span[2 * nb.o + 1]);
            R = a.row.radius[na.o] + a.col.radius[nb.o];
            if (!cp_finite(R)) st = MPCX_ST_NUMERIC;
        }
    }
    const double Rp = fmax(R, 0.0);
    if (st == MPCX_ST_OK) st = ew_g(a.row, a.col, fi, fj, t, a.mu, Rp, a.nsigma, g0);          // the same on every lane
    if (st == MPCX_ST_OK && !cp_finite(g0)) st = MPCX_ST_NUMERIC;
    if (st == MPCX_ST_OK) {
        double reach[2];
        if (g0 > 0.0) {                                                  // clear: t itself is not live, nothing is searched
            double cell = H;
            for (int lv = 0; lv < a.levels; ++lv) cell = cell / 64.0;
            reach[0] = cell; reach[1] = cell;
            fl = MPCX_EW_CLEAR;
        } else {
#pragma unroll 1
            for (int sd = 0; sd < 2; ++sd) {                             // the side before t, then the side after it
                const double sg = sd ? 1.0 : -1.0;
                double lb = 0.0, ub = H;
#pragma unroll 1
                for (int lv = 0; lv < a.levels; ++lv) {
                    const double wd = (ub - lb) / 64.0;
                    const double off = lb + (double)(lane + 1) * wd;
                    double g = 0.0;
                    const int sl = ew_g(a.row, a.col, fi, fj, t + sg * off, a.mu, Rp, a.nsigma, g);
                    // outside a span: not live; numerically bad: cannot be ruled out, live
                    const bool live = sl == MPCX_ST_OK ? g <= 0.0 : sl != MPCX_ST_BADK;
                    if (__any(sl != MPCX_ST_OK && sl != MPCX_ST_BADK)) fl |= MPCX_EW_BAD_SCAN;
                    const unsigned long long dead = __ballot(!live);
                    if (dead == 0ull) {
                        if (lv == 0) fl |= sd ? MPCX_EW_OPEN_AFTER : MPCX_EW_OPEN_BEFORE;
                        break;                                           // (level 0: ub is H; later: ub stays)
                    }
                    const int ls = __ffsll((long long)dead) - 1;
                    const double nl = lb + (double)ls * wd, nu = lb + (double)(ls + 1) * wd;
                    lb = nl; ub = nu;
                }
                reach[sd] = ub;
            }
        }
        o[MPCX_EW_HALF] = fmax(reach[0], reach[1]);
        o[MPCX_EW_TA] = fmax(t - reach[0], lo);
        o[MPCX_EW_TB] = fmin(t + reach[1], hi);
        o[MPCX_EW_REACH_BEFORE] = reach[0];
        o[MPCX_EW_REACH_AFTER] = reach[1];
        o[MPCX_EW_G0] = g0;
    }
    if (lane == 0) {
        double *out = a.out + (size_t)pr * MPCX_NEW;
#pragma unroll
        for (int c = 0; c < MPCX_NEW; ++c) out[c] = o[c];
        a.flags[pr] = fl;
        a.status[pr] = st;
    }
}

// the call as both entry points take it (the names enc_sides reads)
struct EwCall : EncGeometry {
    const double *max_half;
    double nsigma;
    int levels;
    double *out;
    int32_t *flags, *status;
};
#define MPCX_EW_CALL EwCall{MPCX_GEOMETRY(radius, cat_radius), max_half, nsigma, levels, out, flags, status}

static int ew_check(mpcx_ctx *ctx, const EwCall &c)
{
    static const char *const name = "encounter_window";
    if (int rc = geom_check_sizes(ctx, c, name)) return rc;
    if (!(c.nsigma > 0.0) || !(fabs(c.nsigma) < INFINITY)) return enc_fail(ctx, name, "nsigma must be positive and finite");
    if (c.levels < 1 || c.levels > MPCX_EW_MAX_LEVELS) return enc_fail(ctx, name, "levels must be 1..MPCX_EW_MAX_LEVELS");
    return geom_check_arrays(ctx, c, name, true, c.max_half && c.out && c.flags && c.status,
                             "pairs, Y, units, span, P, radius, max_half, out, flags and status");
}

static int ew_enqueue(mpcx_ctx *ctx, const EwCall &c, hipStream_t st)
{
    CpSide row, col;
    enc_sides(c, row, col);
    const EwArgs a{c.n, c.pairs, row, col, c.mu, c.max_half, c.nsigma, c.levels, c.out, c.flags, c.status};
    hipLaunchKernelGGL(encounter_window_kernel, dim3((unsigned)c.n), dim3(64), 0, st, a);
    MPCX_HIP(ctx, hipGetLastError());
    return MPCX_OK;
}

}  // namespace mpcx

using namespace mpcx;

extern "C" int mpcx_encounter_window_dev(mpcx_ctx *ctx, int n, const double *pairs, int S, int K, const int32_t *Ks, const double *Y,
                                         const double *units, const double *span, const double *P, const double *radius, int D, int cat_K,
                                         const int32_t *cat_Ks, const double *cat_Y, const double *cat_units, const double *cat_span,
                                         const double *cat_P, const double *cat_radius, double mu, const double *max_half, double nsigma,
                                         int levels, double *out, int32_t *flags, int32_t *status, void *stream)
{
    if (!ctx) return MPCX_E_BADARG;
    const EwCall c = MPCX_EW_CALL;
    if (int rc = ew_check(ctx, c)) return rc;
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    return ew_enqueue(ctx, c, (hipStream_t)stream);
}

extern "C" int mpcx_encounter_window(mpcx_ctx *ctx, int n, const double *pairs, int S, int K, const int32_t *Ks, const double *Y,
                                     const double *units, const double *span, const double *P, const double *radius, int D, int cat_K,
                                     const int32_t *cat_Ks, const double *cat_Y, const double *cat_units, const double *cat_span,
                                     const double *cat_P, const double *cat_radius, double mu, const double *max_half, double nsigma,
                                     int levels, double *out, int32_t *flags, int32_t *status)
{
    if (!ctx) return MPCX_E_BADARG;
    const EwCall c = MPCX_EW_CALL;
    if (int rc = ew_check(ctx, c)) return rc;
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    DeviceArena ar(ctx);
    EwCall d = c;
    geom_upload(ar, d); d.max_half = ar.upload(max_half, (size_t)n);
    d.out = ar.result(out, (size_t)n * MPCX_NEW);
    d.flags = ar.result(flags, (size_t)n);
    d.status = ar.result(status, (size_t)n);
    return host_run(ctx, ar, 0, [&](void *, hipStream_t st) { return ew_enqueue(ctx, d, st); });
}
#undef MPCX_EW_CALL
