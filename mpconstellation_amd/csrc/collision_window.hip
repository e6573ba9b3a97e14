// collision_window.hip -- the collision probability of listed pairs over a time window (include/mpcx.h:
// mpcx_collision_probability_window*): for encounters too slow for the short-encounter model of collision.hip.
//   collision_window_kernel   for every listed row (i, j, ., t): the probability that the two objects are within R = radius_i +
//                             radius_j at the start of the window [t - h, t + h] (a ball integral of the relative position's
//                             Gaussian) plus the expected number of entries into that sphere during the window (the Rice / Coppola
//                             rate, a sphere integral at every time node), from the time-varying relative state and both objects'
//                             full 6 x 6 covariances.  No encounter plane, no straight line.
// One wave per row; lane l is time node l of the 64-point Gauss-Legendre rule of the current panel and does its own setup at its own
// time (collision_window_device.hpp: cw_node), then the 512 sphere points in a wave-uniform loop (cw_rate).  Panels are a loop.  The
// ball term is dealt over the lanes.  Sums are the xor butterfly, lane 0 stores.  No LDS, no atomics, nothing crosses a workgroup.
// Written for a fixed operation order (tests/collision_window_reference.py follows it line by line).
#include "collision_window_device.hpp"

#include <math.h>

namespace mpcx {

struct CwArgs {
    int n;
    const double *pairs;
    CpSide row, col;
    double mu;
    const double *half;
    int panels;
    double *out;
    int32_t *status;
};

__global__ __launch_bounds__(64) void collision_window_kernel(CwArgs a)
{
    const int pr = blockIdx.x, lane = threadIdx.x;
    if (pr >= a.n) return;
    const double *row = a.pairs + (size_t)pr * 4;
    const double fi = row[0], fj = row[1], t = row[3], h = a.half[pr];
    double o[MPCX_NPW];
#pragma unroll
    for (int c = 0; c < MPCX_NPW; ++c) o[c] = cp_nan();
    // the row's own tests (wave-uniform): both objects at t, the half window, the clipped window, the radius
    int st;
    double ta = 0.0, tb = 0.0, R = 0.0;
    {
        double p[3], v[3];
        CpNode na, nb;
        st = cp_state(a.row, fi, t, p, v, na);
        if (st == MPCX_ST_OK) st = cp_state(a.col, fj, t, p, v, nb);
        if (st == MPCX_ST_OK && !(h > 0.0 && cp_finite(h))) st = MPCX_ST_BADK;
        if (st == MPCX_ST_OK) {
            ta = fmax(fmax(t - h, a.row.span[2 * na.o]), a.col.span[2 * nb.o]);
            tb = fmin(fmin(t + h, a.row.span[2 * na.o + 1]), a.col.span[2 * nb.o + 1]);
            if (!(tb > ta)) st = MPCX_ST_BADK;
            R = a.row.radius[na.o] + a.col.radius[nb.o];
            if (st == MPCX_ST_OK && !cp_finite(R)) st = MPCX_ST_NUMERIC;
        }
    }
    if (st == MPCX_ST_OK && !(R > 0.0)) {
        o[MPCX_PW_P] = 0.0; o[MPCX_PW_START] = 0.0; o[MPCX_PW_ENTRIES] = 0.0; o[MPCX_PW_RATE_MAX] = 0.0;
        o[MPCX_PW_T_RATE_MAX] = ta; o[MPCX_PW_TA] = ta; o[MPCX_PW_TB] = tb;
    } else if (st == MPCX_ST_OK) {
        const double ninf = -__longlong_as_double(0x7ff0000000000000LL);
        const double hp = (tb - ta) / (double)a.panels;
        double entries = 0.0, rmax = ninf, tmax = ta;
        CwNode nd;
        for (int p = 0; p < a.panels && st == MPCX_ST_OK; ++p) {
            const double tau = (ta + (double)p * hp) + (0.5 * hp) * (1.0 + CP_GL[lane][0]);
            const int sl = cw_node(a.row, a.col, fi, fj, tau, a.mu, nd);
            if (__any(sl == MPCX_ST_BADK)) st = MPCX_ST_BADK;
            else if (__any(sl != MPCX_ST_OK)) st = MPCX_ST_NUMERIC;
            if (st != MPCX_ST_OK) break;
            const double rate = cw_rate(nd, R);
            entries = entries + cp_wave_sum(((0.5 * hp) * CP_GL[lane][1]) * rate);
            const double pm = cp_wave_max(rate);
            const double tm = -cp_wave_max(rate == pm ? -tau : ninf);    // the earliest of equal ones
            if (pm > rmax) { rmax = pm; tmax = tm; }
        }
        if (st == MPCX_ST_OK) {
            st = cw_node(a.row, a.col, fi, fj, ta, a.mu, nd);            // the same on every lane
            if (st == MPCX_ST_OK) {
                const double start = nd.cden * cp_wave_sum(cw_ball_share(nd, R, lane));
                const double total = start + entries;
                if (!cp_finite(total)) st = MPCX_ST_NUMERIC;
                else {
                    o[MPCX_PW_P] = fmin(total, 1.0); o[MPCX_PW_START] = start; o[MPCX_PW_ENTRIES] = entries; o[MPCX_PW_RATE_MAX] = rmax;
                    o[MPCX_PW_T_RATE_MAX] = tmax; o[MPCX_PW_TA] = ta; o[MPCX_PW_TB] = tb;
                }
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < MPCX_NPW; ++c) a.out[(size_t)pr * MPCX_NPW + c] = o[c];
        a.status[pr] = st;
    }
}

// the call as both entry points take it
struct CwCall {
    int n;
    const double *pairs;
    int S, K;
    const int32_t *Ks;
    const double *Y, *units, *span, *P, *radius;
    int D, cat_K;
    const int32_t *cat_Ks;
    const double *cat_Y, *cat_units, *cat_span, *cat_P, *cat_radius;
    double mu;
    const double *half;
    int panels;
    double *out;
    int32_t *status;
};

static int cw_check(mpcx_ctx *ctx, const CwCall &c)
{
    if (c.n < 1 || c.S < 1 || c.K < 2 || !(c.mu > 0.0))
        return ctx_fail(ctx, MPCX_E_BADARG, "collision_probability_window: need n>=1, S>=1, K>=2, mu>0");
    if (c.panels < 1 || c.panels > MPCX_PW_MAX_PANELS)
        return ctx_fail(ctx, MPCX_E_BADARG, "collision_probability_window: panels must be 1..MPCX_PW_MAX_PANELS");
    if (!c.pairs || !c.Y || !c.units || !c.span || !c.P || !c.radius || !c.half || !c.out || !c.status)
        return ctx_fail(ctx, MPCX_E_BADARG,
                        "collision_probability_window: pairs, Y, units, span, P, radius, half_window, out and status are required");
    if (c.cat_Y) {
        if (c.D < 1 || c.cat_K < 2) return ctx_fail(ctx, MPCX_E_BADARG, "collision_probability_window: a catalogue needs D>=1, cat_K>=2");
        if (!c.cat_units || !c.cat_span || !c.cat_P || !c.cat_radius)
            return ctx_fail(ctx, MPCX_E_BADARG,
                            "collision_probability_window: cat_units, cat_span, cat_P and cat_radius are required with cat_Y");
    }
    return MPCX_OK;
}

static int cw_enqueue(mpcx_ctx *ctx, const CwCall &c, hipStream_t st)
{
    const CpSide row{c.S, c.K, c.Ks, c.Y, c.units, c.span, c.P, c.radius};
    const CpSide col = c.cat_Y ? CpSide{c.D, c.cat_K, c.cat_Ks, c.cat_Y, c.cat_units, c.cat_span, c.cat_P, c.cat_radius} : row;
    const CwArgs a{c.n, c.pairs, row, col, c.mu, c.half, c.panels, c.out, c.status};
    hipLaunchKernelGGL(collision_window_kernel, dim3((unsigned)c.n), dim3(64), 0, st, a);
    MPCX_HIP(ctx, hipGetLastError());
    return MPCX_OK;
}

}  // namespace mpcx

using namespace mpcx;

extern "C" int mpcx_collision_probability_window_dev(mpcx_ctx *ctx, int n, const double *pairs, int S, int K, const int32_t *Ks,
                                                     const double *Y, const double *units, const double *span, const double *P,
                                                     const double *radius, int D, int cat_K, const int32_t *cat_Ks, const double *cat_Y,
                                                     const double *cat_units, const double *cat_span, const double *cat_P,
                                                     const double *cat_radius, double mu, const double *half_window, int panels,
                                                     double *out, int32_t *status, void *stream)
{
    if (!ctx) return MPCX_E_BADARG;
    const CwCall c{n, pairs, S, K, Ks, Y, units, span, P, radius, D, cat_K, cat_Ks, cat_Y, cat_units, cat_span, cat_P, cat_radius, mu,
                   half_window, panels, out, status};
    if (int rc = cw_check(ctx, c)) return rc;
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    return cw_enqueue(ctx, c, (hipStream_t)stream);
}

extern "C" int mpcx_collision_probability_window(mpcx_ctx *ctx, int n, const double *pairs, int S, int K, const int32_t *Ks, const double *Y,
                                                 const double *units, const double *span, const double *P, const double *radius, int D,
                                                 int cat_K, const int32_t *cat_Ks, const double *cat_Y, const double *cat_units,
                                                 const double *cat_span, const double *cat_P, const double *cat_radius, double mu,
                                                 const double *half_window, int panels, double *out, int32_t *status)
{
    if (!ctx) return MPCX_E_BADARG;
    const CwCall c{n, pairs, S, K, Ks, Y, units, span, P, radius, D, cat_K, cat_Ks, cat_Y, cat_units, cat_span, cat_P, cat_radius, mu,
                   half_window, panels, out, status};
    if (int rc = cw_check(ctx, c)) return rc;
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    DeviceArena ar(ctx);
    CwCall d = c;
    d.pairs = ar.upload(pairs, (size_t)n * 4);
    d.half = ar.upload(half_window, (size_t)n);
    d.Y = ar.upload(Y, (size_t)S * 7 * K); d.units = ar.upload(units, (size_t)S * 2); d.span = ar.upload(span, (size_t)S * 2);
    d.P = ar.upload(P, (size_t)S * K * 36); d.radius = ar.upload(radius, S);
    d.Ks = Ks ? ar.upload(Ks, S) : nullptr;
    if (cat_Y) {
        d.cat_Y = ar.upload(cat_Y, (size_t)D * 7 * cat_K); d.cat_units = ar.upload(cat_units, (size_t)D * 2);
        d.cat_span = ar.upload(cat_span, (size_t)D * 2); d.cat_P = ar.upload(cat_P, (size_t)D * cat_K * 36);
        d.cat_radius = ar.upload(cat_radius, D);
        d.cat_Ks = cat_Ks ? ar.upload(cat_Ks, D) : nullptr;
    }
    d.out = ar.alloc<double>((size_t)n * MPCX_NPW);
    d.status = ar.alloc<int32_t>(n);
    if (ar.failed()) return ar.code();
    if (int rc = cw_enqueue(ctx, d, ctx->stream)) return rc;
    ar.download(out, d.out, (size_t)n * MPCX_NPW);
    ar.download(status, d.status, n);
    return ar.finish();
}
