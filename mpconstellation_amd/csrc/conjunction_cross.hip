// conjunction_cross.hip -- the constellation against a catalogue of foreign objects (include/mpcx.h: mpcx_conjunction_cross_*): rows
// are the constellation's satellites, columns the catalogue's objects, both on the same grid of M common instants.  The rectangle
// S x D is computed, not the square (S + D)^2 of the union.  The arithmetic of a pair is conjunction_common.hpp's, the difference
// always catalogue - satellite: what the all-pairs screen computes for the pair (i, S + j) of the union [constellation; catalogue],
// bit for bit.  Every reduction is a minimum under the total order (squared distance, catalogue index, interval), so nothing
// depends on tiles, grid dimensions, row blocks or device count.
#include "conjunction_common.hpp"

namespace mpcx {

constexpr int CJX_TC = 16;            // columns of a tile: a lane keeps the pair minimum of each in registers while it walks the grid
constexpr int CJX_WAVES = 2048;       // waves the launch aims at: two on each of the 256 x 4 SIMDs, what the kernel's registers admit
constexpr int CJX_WIDE_FROM = 512;    // rows from which a workgroup takes 256 of them (four waves share the staged columns) instead of 64

struct CrossArgs {
    int D, M, row0, nrows, max_pairs;
    double T0, T1, h, thr;
    const double *rowT, *catT;        // instant-major copies: the launch's rows [M][6][nrows], the catalogue [M][6][D]
    double *pd2, *pt;                 // partial row minima [gridDim.y][nrows]: squared distance, time
    int32_t *pj;                      //                                         catalogue index
    double *pairs;                    // [max_pairs][4]
    unsigned long long *count;
};

// One lane per row satellite, a workgroup of ROWS rows (blockIdx.x) that takes the column tiles blockIdx.y, blockIdx.y +
// gridDim.y, ...  As in conjunction_kernel a lane walks all grid intervals for one tile of CJX_TC catalogue objects with the
// tile's pair minima in registers; its own ends come coalesced from rowT once per interval and serve the whole tile, the
// objects' ends are staged in LDS, TM intervals at a time, and read by every lane at the same address (a broadcast).  ROWS and
// gridDim.y are the launch's choice (cross_launch): 64-row workgroups are single waves, so that a few rows against a long
// catalogue still put a wave with 64 live lanes on every SIMD.
template <int ROWS, int TM> __global__ __launch_bounds__(ROWS) void conjunction_cross_kernel(CrossArgs a)
{
    __shared__ double col[(TM + 1) * CJX_TC * 6];                // [instant of the chunk][column][px py pz vx vy vz]
    const int lane = threadIdx.x;
    const int r = blockIdx.x * ROWS + lane;                      // row of the launch's block of rows
    const bool row_ok = r < a.nrows;
    const size_t ir = row_ok ? r : 0;                            // (lanes past the last row load the first row's ends and record nothing)
    const size_t R = (size_t)a.nrows, D = (size_t)a.D;
    double bd2 = cj_inf(), bt = cj_nan();
    int bj = -1;
    const int ntile = (a.D + CJX_TC - 1) / CJX_TC;
    for (int jt = blockIdx.y; jt < ntile; jt += gridDim.y) {
        const int j0 = jt * CJX_TC;
        double pd2[CJX_TC], pt[CJX_TC];
#pragma unroll
        for (int jj = 0; jj < CJX_TC; ++jj) { pd2[jj] = cj_inf(); pt[jj] = cj_nan(); }
        for (int m0 = 0; m0 < a.M - 1; m0 += TM) {
            const int nm = a.M - 1 - m0 < TM ? a.M - 1 - m0 : TM;                // intervals of this chunk
            __syncthreads();
            for (int e = lane; e < (nm + 1) * CJX_TC * 6; e += ROWS) {
                const int mm = e / (CJX_TC * 6), q = e - mm * (CJX_TC * 6), c = q / CJX_TC, jj = q - c * CJX_TC;
                const int j = j0 + jj;
                col[(mm * CJX_TC + jj) * 6 + c] = j < a.D ? a.catT[((size_t)(m0 + mm) * 6 + c) * D + j] : cj_nan();
            }
            __syncthreads();
            double p0[3], v0[3], p1[3], v1[3];
            for (int c = 0; c < 3; ++c) {
                p1[c] = a.rowT[((size_t)m0 * 6 + c) * R + ir];
                v1[c] = a.rowT[((size_t)m0 * 6 + 3 + c) * R + ir];
            }
            for (int mm = 0; mm < nm; ++mm) {
                const int m = m0 + mm;
                for (int c = 0; c < 3; ++c) {
                    p0[c] = p1[c]; v0[c] = v1[c];
                    p1[c] = a.rowT[((size_t)(m + 1) * 6 + c) * R + ir];
                    v1[c] = a.rowT[((size_t)(m + 1) * 6 + 3 + c) * R + ir];
                }
                const double t0 = cj_time(m, a.M, a.T0, a.T1, a.h), t1 = cj_time(m + 1, a.M, a.T0, a.T1, a.h);
#pragma unroll
                for (int jj = 0; jj < CJX_TC; ++jj) {
                    if (!row_ok) continue;
                    const double *c0 = col + (mm * CJX_TC + jj) * 6, *c1 = c0 + CJX_TC * 6;
                    double d0[3], d1[3];
                    for (int c = 0; c < 3; ++c) {
                        d0[c] = c0[c] - p0[c];                                   // catalogue - satellite: the union's higher - lower
                        d1[c] = c1[c] - p1[c];
                    }
                    cj_interval(d0, d1, c0 + 3, c1 + 3, v0, v1, true, a.h, t0, t1, pd2[jj], pt[jj]);
                }
            }
        }
#pragma unroll
        for (int jj = 0; jj < CJX_TC; ++jj) {
            const int j = j0 + jj;
            if (!(pd2[jj] < cj_inf())) continue;                                 // no valid interval for this pair (or j >= D)
            if (pd2[jj] < bd2 || (pd2[jj] == bd2 && j < bj)) { bd2 = pd2[jj]; bt = pt[jj]; bj = j; }
            if (a.thr > 0.0) {
                const double d = sqrt(pd2[jj]);
                if (d <= a.thr) {
                    const unsigned long long at = atomicAdd(a.count, 1ULL);
                    if (at < (unsigned long long)a.max_pairs) {
                        double *o = a.pairs + at * 4;
                        o[0] = (double)(a.row0 + r); o[1] = (double)j; o[2] = d; o[3] = pt[jj];
                    }
                }
            }
        }
    }
    if (row_ok) {
        const size_t at = (size_t)blockIdx.y * a.nrows + r;
        a.pd2[at] = bd2; a.pt[at] = bt; a.pj[at] = bj;
    }
}

// The launch shape from nrows and D: rows per workgroup (256 from CJX_WIDE_FROM rows on, 64 below), and as many column groups as
// it takes to reach CJX_WAVES waves, at most one per column tile.
struct CrossLaunch {
    int rows, rowtiles, groups;
    CrossLaunch(int nrows, int D)
    {
        rows = nrows >= CJX_WIDE_FROM ? 256 : 64;
        rowtiles = (nrows + rows - 1) / rows;
        const int waves = rowtiles * (rows / 64), ntile = (D + CJX_TC - 1) / CJX_TC;
        groups = (CJX_WAVES + waves - 1) / waves;
        if (groups > ntile) groups = ntile;
    }
};

// partial minima of a launch: groups * nrows <= (CJX_WAVES / waves + 1) * nrows, waves >= nrows / 64
static size_t cross_partials(int S) { return (size_t)CJX_WAVES * 64 + (size_t)S + 256; }

// workspace: [rowT M*6*S][catT M*6*D][partial d2][partial t][partial j], and behind them, for the fused call alone (which sizes its
// own), [eph S*6*M][cat D*6*M]: a _dev caller brings its ephemerides and does not pay for a second copy of them
struct CrossWorkspace {
    double *rowT, *catT, *pd2, *pt, *eph, *cat;
    int32_t *pj;
    size_t bytes;
    CrossWorkspace(void *base, int S, int D, int M, bool fused)
    {
        char *p = (char *)base;
        const size_t e = cj_align((size_t)S * 6 * M * sizeof(double)), c = cj_align((size_t)D * 6 * M * sizeof(double));
        const size_t g = cj_align(cross_partials(S) * sizeof(double));
        rowT = (double *)p; p += e;
        catT = (double *)p; p += c;
        pd2 = (double *)p; p += g;
        pt = (double *)p; p += g;
        pj = (int32_t *)p; p += g;
        eph = cat = nullptr;
        if (fused) {
            eph = (double *)p; p += e;
            cat = (double *)p; p += c;
        }
        bytes = (size_t)(p - (char *)base);
    }
};

static int cross_check(mpcx_ctx *ctx, int S, int D, int M, double T0, double T1, int row0, int nrows, double threshold, int max_pairs,
                       const void *pairs, const void *n_pairs)
{
    if (S < 1 || D < 1 || M < 2 || !(T1 > T0) || max_pairs < 0)
        return ctx_fail(ctx, MPCX_E_BADARG, "conjunction_cross_screen: need S>=1, D>=1, M>=2, T1>T0, max_pairs>=0");
    if (row0 < 0 || nrows < 1 || row0 > S - nrows)
        return ctx_fail(ctx, MPCX_E_BADARG, "conjunction_cross_screen: rows row0 .. row0+nrows-1 must lie in 0 .. S-1");
    if (threshold > 0.0 && (!n_pairs || (max_pairs > 0 && !pairs)))
        return ctx_fail(ctx, MPCX_E_BADARG, "conjunction_cross_screen: a threshold needs n_pairs, and pairs when max_pairs > 0");
    return MPCX_OK;
}

}  // namespace mpcx

using namespace mpcx;

extern "C" size_t mpcx_conjunction_cross_workspace_bytes(int S, int D, int M)
{
    if (S < 1 || D < 1 || M < 2) return 0;
    return CrossWorkspace(nullptr, S, D, M, false).bytes;
}

extern "C" int mpcx_conjunction_cross_screen_dev(mpcx_ctx *ctx, int S, int D, int M, const double *eph, const double *cat, double T0,
                                                 double T1, int row0, int nrows, double threshold, int max_pairs, double *dmin,
                                                 int32_t *partner, double *tca, double *pairs, int64_t *n_pairs, void *workspace,
                                                 void *stream)
{
    if (!ctx) return MPCX_E_BADARG;
    if (int rc = cross_check(ctx, S, D, M, T0, T1, row0, nrows, threshold, max_pairs, pairs, n_pairs)) return rc;
    if (!eph || !cat || !dmin || !partner || !tca || !workspace)
        return ctx_fail(ctx, MPCX_E_BADARG, "conjunction_cross_screen: eph, cat, dmin, partner, tca and workspace are required");
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    CrossWorkspace ws(workspace, S, D, M, false);
    // the launch's rows alone, and the whole catalogue (once per call)
    const long rtotal = (long)nrows * M, ctotal = (long)D * M;
    hipLaunchKernelGGL(conjunction_transpose_kernel, dim3((unsigned)((rtotal + 255) / 256)), dim3(256), 0, st, nrows, M,
                       eph + (size_t)row0 * 6 * M, ws.rowT);
    MPCX_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(conjunction_transpose_kernel, dim3((unsigned)((ctotal + 255) / 256)), dim3(256), 0, st, D, M, cat, ws.catT);
    MPCX_HIP(ctx, hipGetLastError());
    if (n_pairs) MPCX_HIP(ctx, hipMemsetAsync(n_pairs, 0, sizeof(int64_t), st));
    const CrossLaunch L(nrows, D);
    CrossArgs a{D, M, row0, nrows, max_pairs, T0, T1, (T1 - T0) / (double)(M - 1), threshold > 0.0 ? threshold : 0.0, ws.rowT, ws.catT,
                ws.pd2, ws.pt, ws.pj, pairs, (unsigned long long *)n_pairs};
    const dim3 grid((unsigned)L.rowtiles, (unsigned)L.groups);
    if (L.rows == 256) hipLaunchKernelGGL((conjunction_cross_kernel<256, 32>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((conjunction_cross_kernel<64, 16>), grid, dim3(64), 0, st, a);
    MPCX_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(conjunction_reduce_kernel, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, st, nrows, L.groups, ws.pd2, ws.pt, ws.pj,
                       dmin, partner, tca);
    MPCX_HIP(ctx, hipGetLastError());
    return MPCX_OK;
}

// the part the two host-pointer screens share: both ephemerides already in HBM -> results in the caller's arrays
static int cross_screen_from_device(mpcx_ctx *ctx, DeviceArena &ar, int S, int D, int M, const double *deph, const double *dcat, void *dws,
                                    double T0, double T1, int row0, int nrows, double threshold, int max_pairs, double *dmin,
                                    int32_t *partner, double *tca, double *pairs, int64_t *n_pairs)
{
    const bool list = threshold > 0.0;
    double *dd = ar.alloc<double>(nrows), *dt = ar.alloc<double>(nrows);
    int32_t *dp = ar.alloc<int32_t>(nrows);
    double *dpairs = list && max_pairs > 0 ? ar.alloc<double>((size_t)max_pairs * 4) : nullptr;
    int64_t *dn = ar.alloc<int64_t>(1);
    if (ar.failed()) return ar.code();
    if (dpairs) MPCX_HIP(ctx, hipMemsetAsync(dpairs, 0, (size_t)max_pairs * 4 * sizeof(double), ctx->stream));
    if (int rc = mpcx_conjunction_cross_screen_dev(ctx, S, D, M, deph, dcat, T0, T1, row0, nrows, threshold, max_pairs, dd, dp, dt, dpairs, dn,
                                                   dws, ctx->stream))
        return rc;
    ar.download(dmin, dd, nrows); ar.download(partner, dp, nrows); ar.download(tca, dt, nrows);
    if (dpairs) ar.download(pairs, dpairs, (size_t)max_pairs * 4);
    if (n_pairs) ar.download(n_pairs, dn, 1);
    return ar.finish();
}

extern "C" int mpcx_conjunction_cross_screen(mpcx_ctx *ctx, int S, int D, int M, const double *eph, const double *cat, double T0, double T1,
                                             int row0, int nrows, double threshold, int max_pairs, double *dmin, int32_t *partner,
                                             double *tca, double *pairs, int64_t *n_pairs)
{
    if (!ctx) return MPCX_E_BADARG;
    if (int rc = cross_check(ctx, S, D, M, T0, T1, row0, nrows, threshold, max_pairs, pairs, n_pairs)) return rc;
    if (!eph || !cat || !dmin || !partner || !tca)
        return ctx_fail(ctx, MPCX_E_BADARG, "conjunction_cross_screen: eph, cat, dmin, partner and tca are required");
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    DeviceArena ar(ctx);
    double *de = ar.upload(eph, (size_t)S * 6 * M), *dc = ar.upload(cat, (size_t)D * 6 * M);
    char *dws = ar.alloc<char>(mpcx_conjunction_cross_workspace_bytes(S, D, M));
    if (ar.failed()) return ar.code();
    return cross_screen_from_device(ctx, ar, S, D, M, de, dc, dws, T0, T1, row0, nrows, threshold, max_pairs, dmin, partner, tca, pairs, n_pairs);
}

extern "C" int mpcx_conjunction_cross_screen_traj(mpcx_ctx *ctx, int S, int n, const int32_t *ns, const double *Y, const double *units,
                                                  const double *span, int D, int cat_n, const int32_t *cat_ns, const double *cat_Y,
                                                  const double *cat_units, const double *cat_span, int M, double T0, double T1, int row0,
                                                  int nrows, double threshold, int max_pairs, double *dmin, int32_t *partner, double *tca,
                                                  double *pairs, int64_t *n_pairs, int32_t *status, int32_t *cat_status)
{
    if (!ctx) return MPCX_E_BADARG;
    if (S < 1 || D < 1 || M < 2 || n < 1 || cat_n < 1 || !(T1 > T0))
        return ctx_fail(ctx, MPCX_E_BADARG, "conjunction_cross_screen_traj: need S>=1, D>=1, n>=1, cat_n>=1, M>=2, T1>T0");
    if (int rc = cross_check(ctx, S, D, M, T0, T1, row0, nrows, threshold, max_pairs, pairs, n_pairs)) return rc;
    if (!Y || !units || !span || !cat_Y || !cat_units || !cat_span || !dmin || !partner || !tca)
        return ctx_fail(ctx, MPCX_E_BADARG,
                        "conjunction_cross_screen_traj: Y, units, span, cat_Y, cat_units, cat_span, dmin, partner and tca are required");
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    DeviceArena ar(ctx);
    double *dY = ar.upload(Y, (size_t)S * 7 * n), *du = ar.upload(units, (size_t)S * 2), *dsp = ar.upload(span, (size_t)S * 2);
    int32_t *dns = ns ? ar.upload(ns, S) : nullptr;
    double *cY = ar.upload(cat_Y, (size_t)D * 7 * cat_n), *cu = ar.upload(cat_units, (size_t)D * 2), *csp = ar.upload(cat_span, (size_t)D * 2);
    int32_t *cns = cat_ns ? ar.upload(cat_ns, D) : nullptr;
    int32_t *dst = ar.alloc<int32_t>(S), *cst = ar.alloc<int32_t>(D);
    char *dws = ar.alloc<char>(CrossWorkspace(nullptr, S, D, M, true).bytes);  // the screen's workspace, then the two ephemerides
    if (ar.failed()) return ar.code();
    const CrossWorkspace ws(dws, S, D, M, true);                             // neither ephemeris leaves HBM
    if (int rc = mpcx_ephemeris_batch_dev(ctx, S, n, dns, dY, du, dsp, M, T0, T1, ws.eph, dst, ctx->stream)) return rc;
    if (int rc = mpcx_ephemeris_batch_dev(ctx, D, cat_n, cns, cY, cu, csp, M, T0, T1, ws.cat, cst, ctx->stream)) return rc;
    if (status) ar.download(status, dst, S);
    if (cat_status) ar.download(cat_status, cst, D);
    return cross_screen_from_device(ctx, ar, S, D, M, ws.eph, ws.cat, dws, T0, T1, row0, nrows, threshold, max_pairs, dmin, partner, tca,
                                    pairs, n_pairs);
}
