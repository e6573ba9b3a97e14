// conjunction_common.hpp -- what the two screens share (conjunction.hip: every pair of one constellation; conjunction_cross.hip:
// a constellation against a foreign catalogue): the grid's instants, the closest approach of two Hermite arcs inside one grid
// interval, the instant-major copy of an ephemeris and the reduction of the column groups' partial row minima.  One text, so that
// a pair gets the same bits whichever screen looks at it.  The kernels are static: every translation unit that includes this
// file gets its own copy.
#pragma once
#include "mpcx_host.hpp"

#include <math.h>

namespace mpcx {

__device__ __forceinline__ double cj_nan() { return __longlong_as_double(0x7ff8000000000000LL); }
__device__ __forceinline__ double cj_inf() { return __longlong_as_double(0x7ff0000000000000LL); }

// np.linspace(T0, T1, M)[m]: m * step, the last instant exactly T1 (a satellite whose span ends at T1 is still inside)
__device__ __forceinline__ double cj_time(int m, int M, double T0, double T1, double h)
{
    return m == M - 1 ? T1 : T0 + (double)m * h;
}

// eph [S][6][M] -> the screen's instant-major copy ephT [M][6][S] (the rows of one instant side by side: a row tile's loads
// are coalesced, an instant's S x 48 B stay in L2 across the row tiles).  An end with a NaN in any of its six values becomes
// NaN in all six, so that the screen tests positions only.  One lane per (instant, satellite).
static __global__ __launch_bounds__(256) void conjunction_transpose_kernel(int S, int M, const double *eph, double *ephT)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)S * M) return;
    const int m = (int)(idx / S), s = (int)(idx - (long)m * S);
    double v[6];
    bool nan = false;
    for (int c = 0; c < 6; ++c) { v[c] = eph[((size_t)s * 6 + c) * M + m]; nan = nan || !(v[c] == v[c]); }
    for (int c = 0; c < 6; ++c) ephT[((size_t)m * 6 + c) * S + s] = nan ? cj_nan() : v[c];
}

__device__ __forceinline__ double cj_dot(const double (&a)[3], const double (&b)[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// The closest approach of one pair inside one grid interval.  d0, d1: hi - lo position differences at the interval's ends;
// cv0, cv1 / v0, v1: the column's and the row's velocities there (their difference, hi - lo, is formed only where the Newton
// steps need it; up: the column is the higher index).  Distances are compared squared (the root is taken once, on the way out).  Updates
// (best, tbest) when the interval comes closer: ends first, the interior point last, each only if strictly smaller.
__device__ __forceinline__ void cj_interval(const double (&d0)[3], const double (&d1)[3], const double *cv0, const double *cv1,
                                            const double (&v0)[3], const double (&v1)[3], bool up, double h, double t0, double t1,
                                            double &best, double &tbest)
{
    const double q0 = cj_dot(d0, d0), q1 = cj_dot(d1, d1);
    if (!(q0 == q0) || !(q1 == q1)) return;                       // an end outside a satellite's span
    double q = q0, tq = t0;
    if (q1 < q) { q = q1; tq = t1; }
    const double D[3] = {d1[0] - d0[0], d1[1] - d0[1], d1[2] - d0[2]};
    const double DD = cj_dot(D, D), b = cj_dot(d0, D);
    double s = 0.0;
    if (DD > 0.0 && DD < cj_inf()) {
        s = -b / DD;
        s = s < 0.0 ? 0.0 : (s > 1.0 ? 1.0 : s);
    }
    if (s > 0.0 && s < 1.0) {
        double a0[3], a1[3];                                      // h w0, h w1
        for (int c = 0; c < 3; ++c) {
            a0[c] = h * (up ? cv0[c] - v0[c] : v0[c] - cv0[c]);
            a1[c] = h * (up ? cv1[c] - v1[c] : v1[c] - cv1[c]);
        }
        double x[3];
        for (int it = 0; it < 4; ++it) {                          // three Newton steps, then the distance at the result
            const double s2 = s * s, s3 = s2 * s;
            const double h00 = 2.0 * s3 - 3.0 * s2 + 1.0, h10 = s3 - 2.0 * s2 + s, h01 = -2.0 * s3 + 3.0 * s2, h11 = s3 - s2;
            for (int c = 0; c < 3; ++c) x[c] = h00 * d0[c] + h10 * a0[c] + h01 * d1[c] + h11 * a1[c];
            if (it == 3) break;
            const double g00 = 6.0 * s2 - 6.0 * s, g10 = 3.0 * s2 - 4.0 * s + 1.0, g01 = -6.0 * s2 + 6.0 * s, g11 = 3.0 * s2 - 2.0 * s;
            const double k00 = 12.0 * s - 6.0, k10 = 6.0 * s - 4.0, k01 = -12.0 * s + 6.0, k11 = 6.0 * s - 2.0;
            double x1[3], x2[3];
            for (int c = 0; c < 3; ++c) {
                x1[c] = g00 * d0[c] + g10 * a0[c] + g01 * d1[c] + g11 * a1[c];
                x2[c] = k00 * d0[c] + k10 * a0[c] + k01 * d1[c] + k11 * a1[c];
            }
            const double g = cj_dot(x, x1), gp = cj_dot(x1, x1) + cj_dot(x, x2);
            if (gp > 0.0) {
                s = s - g / gp;
                s = s < 0.0 ? 0.0 : (s > 1.0 ? 1.0 : s);
            }
        }
        const double qs = cj_dot(x, x);
        if (qs < q) { q = qs; tq = t0 + s * h; }
    }
    if (q < best) { best = q; tbest = tq; }
}

// the column groups' partial minima of every row -> dmin, partner, tca (a minimum under (distance, partner): any order gives it)
static __global__ __launch_bounds__(256) void conjunction_reduce_kernel(int nrows, int ngroups, const double *pd2, const double *pt, const int32_t *pj,
                                                                 double *dmin, int32_t *partner, double *tca)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= nrows) return;
    double bd2 = cj_inf(), bt = cj_nan();
    int bj = -1;
    for (int g = 0; g < ngroups; ++g) {
        const size_t at = (size_t)g * nrows + r;
        const int j = pj[at];
        if (j < 0) continue;
        const double d2 = pd2[at];
        if (bj < 0 || d2 < bd2 || (d2 == bd2 && j < bj)) { bd2 = d2; bt = pt[at]; bj = j; }
    }
    dmin[r] = bj < 0 ? cj_inf() : sqrt(bd2);
    partner[r] = bj;
    tca[r] = bt;
}

static inline size_t cj_align(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace mpcx
