// conjunction.hip -- the constellation on one clock, and the all-pairs closest approach on it (include/mpcx.h: mpcx_ephemeris_*,
// mpcx_conjunction_*).  Every other kernel of the library works on one satellite in its own units (SatelliteScale: length = its
// start radius, time = its own period), so node k of two satellites is two different instants in two different lengths.  Here
//   ephemeris_kernel     resamples every trajectory at M common instants in metres and m/s: cubic Hermite in physical time on the
//                        node positions and velocities (the state carries the velocity: C1, error h_n^4 / 384 max |p''''|);
//   conjunction_kernel   for every ordered pair (i, j != i) and every grid interval the closest approach of the two Hermite
//                        arcs -- chord minimum, then three Newton steps on d . d' -- reduced to one (distance, partner, time) per
//                        row and, with a threshold, to a list of the pairs i < j that come closer than it.
// Arithmetic that both orderings of a pair share: the difference is always (higher index) - (lower index), so (i, j) and (j, i)
// run the same operations on the same operands and get the same bits; every reduction is a minimum under a total order
// (distance, then partner index, then interval), so nothing depends on tiles, grid dimensions or device count.
#include "conjunction_common.hpp"

namespace mpcx {

constexpr int CJ_ROWS = 256;      // row satellites of a workgroup, one per lane
constexpr int CJ_TC = 16;         // columns of a tile: a lane keeps the pair minimum of each in registers while it walks the grid
constexpr int CJ_TM = 32;         // grid intervals staged in LDS at a time (TM + 1 instants)
constexpr int CJ_MAXGROUPS = 64;  // column groups (gridDim.y) at the most: rows of partial minima in the workspace

struct EphArgs {
    int S, n, M;
    const int32_t *ns;
    const double *Y, *units, *span;
    double T0, T1, h;
    double *eph;
    int32_t *status;
};

// One lane per (satellite, instant); consecutive lanes write consecutive instants of one row of eph [S][6][M].
__global__ __launch_bounds__(256) void ephemeris_kernel(EphArgs a)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)a.S * a.M) return;
    const int s = (int)(idx / a.M), m = (int)(idx - (long)s * a.M);
    const int nn = a.ns ? a.ns[s] : a.n;
    const double ta = a.span[2 * s], tb = a.span[2 * s + 1];
    const bool bad = nn < 2 || nn > a.n || !(tb > ta);
    if (m == 0) a.status[s] = bad ? MPCX_ST_BADK : MPCX_ST_OK;
    double o[6];
    for (int c = 0; c < 6; ++c) o[c] = cj_nan();
    const double t = cj_time(m, a.M, a.T0, a.T1, a.h);
    if (!bad && t >= ta && t <= tb) {
        const double hn = (tb - ta) / (double)(nn - 1);
        const double u = (t - ta) / hn;
        int k = (int)u;
        if (k > nn - 2) k = nn - 2;
        if (k < 0) k = 0;
        const double sg = u - (double)k, s2 = sg * sg, s3 = s2 * sg;
        const double h00 = 2.0 * s3 - 3.0 * s2 + 1.0, h10 = s3 - 2.0 * s2 + sg, h01 = -2.0 * s3 + 3.0 * s2, h11 = s3 - s2;
        const double g00 = 6.0 * s2 - 6.0 * sg, g10 = 3.0 * s2 - 4.0 * sg + 1.0, g01 = -6.0 * s2 + 6.0 * sg, g11 = 3.0 * s2 - 2.0 * sg;
        const double L = a.units[2 * s], V = L / a.units[2 * s + 1];
        const double *y = a.Y + (size_t)s * 7 * a.n;
        for (int c = 0; c < 3; ++c) {
            const double p0 = y[(size_t)c * a.n + k] * L, p1 = y[(size_t)c * a.n + k + 1] * L;
            const double m0 = hn * (y[(size_t)(3 + c) * a.n + k] * V), m1 = hn * (y[(size_t)(3 + c) * a.n + k + 1] * V);
            o[c] = h00 * p0 + h10 * m0 + h01 * p1 + h11 * m1;
            o[3 + c] = (g00 * p0 + g10 * m0 + g01 * p1 + g11 * m1) / hn;
        }
    }
    for (int c = 0; c < 6; ++c) a.eph[((size_t)s * 6 + c) * a.M + m] = o[c];
}

struct ConjArgs {
    int S, M, row0, nrows, max_pairs;
    double T0, T1, h, thr;
    const double *ephT;
    double *pd2, *pt;                 // partial row minima [gridDim.y][nrows]: squared distance, time
    int32_t *pj;                      //                                         partner
    double *pairs;                    // [max_pairs][4]
    unsigned long long *count;
};

// One lane per row satellite, a workgroup of CJ_ROWS rows (blockIdx.x) that takes the column tiles blockIdx.y, blockIdx.y +
// gridDim.y, ...  For one tile of CJ_TC columns a lane walks all grid intervals with the tile's pair minima in registers (the
// minimum of a PAIR over the whole grid is what the pairs list needs); its own ends come from global memory once per interval
// and serve the whole tile, the columns' ends are staged in LDS, CJ_TM intervals at a time, and read by every lane at the same
// address (a broadcast, no bank conflict).  The full square is computed: a row's minimum needs no atomics.
__global__ __launch_bounds__(CJ_ROWS) void conjunction_kernel(ConjArgs a)
{
    __shared__ double col[(CJ_TM + 1) * CJ_TC * 6];              // [instant of the chunk][column][px py pz vx vy vz]
    const int lane = threadIdx.x;
    const int r = blockIdx.x * CJ_ROWS + lane;                   // row of the launch's block of rows
    const bool row_ok = r < a.nrows;
    const int i = a.row0 + (row_ok ? r : 0);                     // (lanes past the last row load row0's ends and record nothing)
    const size_t S = (size_t)a.S;
    double bd2 = cj_inf(), bt = cj_nan();
    int bj = -1;
    const int ntile = (a.S + CJ_TC - 1) / CJ_TC;
    for (int jt = blockIdx.y; jt < ntile; jt += gridDim.y) {
        const int j0 = jt * CJ_TC;
        double pd2[CJ_TC], pt[CJ_TC];
#pragma unroll
        for (int jj = 0; jj < CJ_TC; ++jj) { pd2[jj] = cj_inf(); pt[jj] = cj_nan(); }
        for (int m0 = 0; m0 < a.M - 1; m0 += CJ_TM) {
            const int nm = a.M - 1 - m0 < CJ_TM ? a.M - 1 - m0 : CJ_TM;        // intervals of this chunk
            __syncthreads();
            for (int e = lane; e < (nm + 1) * CJ_TC * 6; e += CJ_ROWS) {
                const int mm = e / (CJ_TC * 6), q = e - mm * (CJ_TC * 6), c = q / CJ_TC, jj = q - c * CJ_TC;
                const int j = j0 + jj;
                col[(mm * CJ_TC + jj) * 6 + c] = j < a.S ? a.ephT[((size_t)(m0 + mm) * 6 + c) * S + j] : cj_nan();
            }
            __syncthreads();
            double p0[3], v0[3], p1[3], v1[3];
            for (int c = 0; c < 3; ++c) {
                p1[c] = a.ephT[((size_t)m0 * 6 + c) * S + i];
                v1[c] = a.ephT[((size_t)m0 * 6 + 3 + c) * S + i];
            }
            for (int mm = 0; mm < nm; ++mm) {
                const int m = m0 + mm;
                for (int c = 0; c < 3; ++c) {
                    p0[c] = p1[c]; v0[c] = v1[c];
                    p1[c] = a.ephT[((size_t)(m + 1) * 6 + c) * S + i];
                    v1[c] = a.ephT[((size_t)(m + 1) * 6 + 3 + c) * S + i];
                }
                const double t0 = cj_time(m, a.M, a.T0, a.T1, a.h), t1 = cj_time(m + 1, a.M, a.T0, a.T1, a.h);
#pragma unroll
                for (int jj = 0; jj < CJ_TC; ++jj) {
                    const int j = j0 + jj;
                    if (j == i || !row_ok) continue;
                    const double *c0 = col + (mm * CJ_TC + jj) * 6, *c1 = c0 + CJ_TC * 6;
                    const bool up = j > i;                                       // the column is the higher index: column - row
                    double d0[3], d1[3];
                    for (int c = 0; c < 3; ++c) {
                        d0[c] = up ? c0[c] - p0[c] : p0[c] - c0[c];
                        d1[c] = up ? c1[c] - p1[c] : p1[c] - c1[c];
                    }
                    cj_interval(d0, d1, c0 + 3, c1 + 3, v0, v1, up, a.h, t0, t1, pd2[jj], pt[jj]);
                }
            }
        }
#pragma unroll
        for (int jj = 0; jj < CJ_TC; ++jj) {
            const int j = j0 + jj;
            if (!(pd2[jj] < cj_inf())) continue;                                 // no valid interval for this pair (or j == i, j >= S)
            if (pd2[jj] < bd2 || (pd2[jj] == bd2 && j < bj)) { bd2 = pd2[jj]; bt = pt[jj]; bj = j; }
            if (a.thr > 0.0 && j > i) {
                const double d = sqrt(pd2[jj]);
                if (d <= a.thr) {
                    const unsigned long long at = atomicAdd(a.count, 1ULL);
                    if (at < (unsigned long long)a.max_pairs) {
                        double *o = a.pairs + at * 4;
                        o[0] = (double)i; o[1] = (double)j; o[2] = d; o[3] = pt[jj];
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

// workspace: [ephT M*6*S][partial d2][partial t][partial j][eph S*6*M, the fused call's]
struct ConjWorkspace {
    double *ephT, *pd2, *pt, *eph;
    int32_t *pj;
    size_t bytes;
    ConjWorkspace(void *base, int S, int M)
    {
        char *p = (char *)base;
        const size_t e = cj_align((size_t)S * 6 * M * sizeof(double)), g = cj_align((size_t)CJ_MAXGROUPS * S * sizeof(double));
        ephT = (double *)p; p += e;
        pd2 = (double *)p; p += g;
        pt = (double *)p; p += g;
        pj = (int32_t *)p; p += g;
        eph = (double *)p; p += e;
        bytes = (size_t)(p - (char *)base);
    }
};

static int conj_check(mpcx_ctx *ctx, int S, int M, double T0, double T1, int row0, int nrows, double threshold, int max_pairs,
                      const void *pairs, const void *n_pairs)
{
    if (S < 1 || M < 2 || !(T1 > T0) || max_pairs < 0)
        return ctx_fail(ctx, MPCX_E_BADARG, "conjunction_screen: need S>=1, M>=2, T1>T0, max_pairs>=0");
    if (row0 < 0 || nrows < 1 || row0 > S - nrows) return ctx_fail(ctx, MPCX_E_BADARG, "conjunction_screen: rows row0 .. row0+nrows-1 must lie in 0 .. S-1");
    if (threshold > 0.0 && (!n_pairs || (max_pairs > 0 && !pairs)))
        return ctx_fail(ctx, MPCX_E_BADARG, "conjunction_screen: a threshold needs n_pairs, and pairs when max_pairs > 0");
    return MPCX_OK;
}

static int eph_check(mpcx_ctx *ctx, int S, int n, int M, double T0, double T1)
{
    if (S < 1 || M < 2 || n < 1 || !(T1 > T0)) return ctx_fail(ctx, MPCX_E_BADARG, "ephemeris: need S>=1, n>=1, M>=2, T1>T0");
    return MPCX_OK;
}

}  // namespace mpcx

using namespace mpcx;

extern "C" size_t mpcx_conjunction_workspace_bytes(int S, int M)
{
    if (S < 1 || M < 2) return 0;
    return ConjWorkspace(nullptr, S, M).bytes;
}

extern "C" int mpcx_ephemeris_batch_dev(mpcx_ctx *ctx, int S, int n, const int32_t *ns, const double *Y, const double *units,
                                        const double *span, int M, double T0, double T1, double *eph, int32_t *status, void *stream)
{
    if (!ctx) return MPCX_E_BADARG;
    if (int rc = eph_check(ctx, S, n, M, T0, T1)) return rc;
    if (!Y || !units || !span || !eph || !status) return ctx_fail(ctx, MPCX_E_BADARG, "ephemeris: Y, units, span, eph and status are required");
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    EphArgs a{S, n, M, ns, Y, units, span, T0, T1, (T1 - T0) / (double)(M - 1), eph, status};
    const long total = (long)S * M;
    hipLaunchKernelGGL(ephemeris_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    MPCX_HIP(ctx, hipGetLastError());
    return MPCX_OK;
}

extern "C" int mpcx_conjunction_screen_dev(mpcx_ctx *ctx, int S, int M, const double *eph, double T0, double T1, int row0, int nrows,
                                           double threshold, int max_pairs, double *dmin, int32_t *partner, double *tca, double *pairs,
                                           int64_t *n_pairs, void *workspace, void *stream)
{
    if (!ctx) return MPCX_E_BADARG;
    if (int rc = conj_check(ctx, S, M, T0, T1, row0, nrows, threshold, max_pairs, pairs, n_pairs)) return rc;
    if (!eph || !dmin || !partner || !tca || !workspace) return ctx_fail(ctx, MPCX_E_BADARG, "conjunction_screen: eph, dmin, partner, tca and workspace are required");
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    ConjWorkspace ws(workspace, S, M);
    const long total = (long)S * M;
    hipLaunchKernelGGL(conjunction_transpose_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, S, M, eph, ws.ephT);
    MPCX_HIP(ctx, hipGetLastError());
    if (n_pairs) MPCX_HIP(ctx, hipMemsetAsync(n_pairs, 0, sizeof(int64_t), st));
    // enough workgroups to fill the device (about four per compute unit) whatever the number of row tiles, at most one per column tile
    const int rowtiles = (nrows + CJ_ROWS - 1) / CJ_ROWS, ntile = (S + CJ_TC - 1) / CJ_TC;
    int groups = (1024 + rowtiles - 1) / rowtiles;
    if (groups > ntile) groups = ntile;
    if (groups > CJ_MAXGROUPS) groups = CJ_MAXGROUPS;
    ConjArgs a{S, M, row0, nrows, max_pairs, T0, T1, (T1 - T0) / (double)(M - 1), threshold > 0.0 ? threshold : 0.0, ws.ephT,
               ws.pd2, ws.pt, ws.pj, pairs, (unsigned long long *)n_pairs};
    hipLaunchKernelGGL(conjunction_kernel, dim3((unsigned)rowtiles, (unsigned)groups), dim3(CJ_ROWS), 0, st, a);
    MPCX_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(conjunction_reduce_kernel, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, st, nrows, groups, ws.pd2, ws.pt, ws.pj,
                       dmin, partner, tca);
    MPCX_HIP(ctx, hipGetLastError());
    return MPCX_OK;
}

extern "C" int mpcx_ephemeris_batch(mpcx_ctx *ctx, int S, int n, const int32_t *ns, const double *Y, const double *units,
                                    const double *span, int M, double T0, double T1, double *eph, int32_t *status)
{
    if (!ctx) return MPCX_E_BADARG;
    if (int rc = eph_check(ctx, S, n, M, T0, T1)) return rc;
    if (!Y || !units || !span || !eph || !status) return ctx_fail(ctx, MPCX_E_BADARG, "ephemeris: Y, units, span, eph and status are required");
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    DeviceArena ar(ctx);
    double *dY = ar.upload(Y, (size_t)S * 7 * n), *du = ar.upload(units, (size_t)S * 2), *dsp = ar.upload(span, (size_t)S * 2);
    int32_t *dns = ns ? ar.upload(ns, S) : nullptr;
    double *de = ar.alloc<double>((size_t)S * 6 * M);
    int32_t *dst = ar.alloc<int32_t>(S);
    if (ar.failed()) return ar.code();
    if (int rc = mpcx_ephemeris_batch_dev(ctx, S, n, dns, dY, du, dsp, M, T0, T1, de, dst, ctx->stream)) return rc;
    ar.download(eph, de, (size_t)S * 6 * M);
    ar.download(status, dst, S);
    return ar.finish();
}

// the part the two host-pointer screens share: eph already in HBM -> results in the caller's arrays
static int conj_screen_from_device(mpcx_ctx *ctx, DeviceArena &ar, int S, int M, const double *deph, void *dws, double T0, double T1, int row0,
                                   int nrows, double threshold, int max_pairs, double *dmin, int32_t *partner, double *tca, double *pairs,
                                   int64_t *n_pairs)
{
    const bool list = threshold > 0.0;
    double *dd = ar.alloc<double>(nrows), *dt = ar.alloc<double>(nrows);
    int32_t *dp = ar.alloc<int32_t>(nrows);
    double *dpairs = list && max_pairs > 0 ? ar.alloc<double>((size_t)max_pairs * 4) : nullptr;
    int64_t *dn = ar.alloc<int64_t>(1);
    if (ar.failed()) return ar.code();
    if (dpairs) MPCX_HIP(ctx, hipMemsetAsync(dpairs, 0, (size_t)max_pairs * 4 * sizeof(double), ctx->stream));
    if (int rc = mpcx_conjunction_screen_dev(ctx, S, M, deph, T0, T1, row0, nrows, threshold, max_pairs, dd, dp, dt, dpairs, dn, dws, ctx->stream))
        return rc;
    ar.download(dmin, dd, nrows); ar.download(partner, dp, nrows); ar.download(tca, dt, nrows);
    if (dpairs) ar.download(pairs, dpairs, (size_t)max_pairs * 4);
    if (n_pairs) ar.download(n_pairs, dn, 1);
    return ar.finish();
}

extern "C" int mpcx_conjunction_screen(mpcx_ctx *ctx, int S, int M, const double *eph, double T0, double T1, int row0, int nrows,
                                       double threshold, int max_pairs, double *dmin, int32_t *partner, double *tca, double *pairs,
                                       int64_t *n_pairs)
{
    if (!ctx) return MPCX_E_BADARG;
    if (int rc = conj_check(ctx, S, M, T0, T1, row0, nrows, threshold, max_pairs, pairs, n_pairs)) return rc;
    if (!eph || !dmin || !partner || !tca) return ctx_fail(ctx, MPCX_E_BADARG, "conjunction_screen: eph, dmin, partner and tca are required");
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    DeviceArena ar(ctx);
    double *de = ar.upload(eph, (size_t)S * 6 * M);
    char *dws = ar.alloc<char>(mpcx_conjunction_workspace_bytes(S, M));
    if (ar.failed()) return ar.code();
    return conj_screen_from_device(ctx, ar, S, M, de, dws, T0, T1, row0, nrows, threshold, max_pairs, dmin, partner, tca, pairs, n_pairs);
}

extern "C" int mpcx_conjunction_screen_traj(mpcx_ctx *ctx, int S, int n, const int32_t *ns, const double *Y, const double *units,
                                            const double *span, int M, double T0, double T1, int row0, int nrows, double threshold,
                                            int max_pairs, double *dmin, int32_t *partner, double *tca, double *pairs, int64_t *n_pairs,
                                            int32_t *status)
{
    if (!ctx) return MPCX_E_BADARG;
    if (int rc = eph_check(ctx, S, n, M, T0, T1)) return rc;
    if (int rc = conj_check(ctx, S, M, T0, T1, row0, nrows, threshold, max_pairs, pairs, n_pairs)) return rc;
    if (!Y || !units || !span || !dmin || !partner || !tca) return ctx_fail(ctx, MPCX_E_BADARG, "conjunction_screen_traj: Y, units, span, dmin, partner and tca are required");
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    DeviceArena ar(ctx);
    double *dY = ar.upload(Y, (size_t)S * 7 * n), *du = ar.upload(units, (size_t)S * 2), *dsp = ar.upload(span, (size_t)S * 2);
    int32_t *dns = ns ? ar.upload(ns, S) : nullptr;
    int32_t *dst = ar.alloc<int32_t>(S);
    char *dws = ar.alloc<char>(mpcx_conjunction_workspace_bytes(S, M));
    if (ar.failed()) return ar.code();
    double *de = ConjWorkspace(dws, S, M).eph;                       // the ephemeris never leaves HBM
    if (int rc = mpcx_ephemeris_batch_dev(ctx, S, n, dns, dY, du, dsp, M, T0, T1, de, dst, ctx->stream)) return rc;
    if (status) ar.download(status, dst, S);
    return conj_screen_from_device(ctx, ar, S, M, de, dws, T0, T1, row0, nrows, threshold, max_pairs, dmin, partner, tca, pairs, n_pairs);
}
