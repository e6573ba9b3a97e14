// conjunction.hip -- the constellation on one clock, and the closest approach of pairs on it (include/mpcx.h: mpcx_ephemeris_*,
// mpcx_conjunction_*, mpcx_conjunction_cross_*).  Every other kernel of the library works on one satellite in its own units
// (SatelliteScale: length = its start radius, time = its own period), so node k of two satellites is two different instants in
// two different lengths.  Here
//   ephemeris_kernel   resamples every trajectory at M common instants in metres and m/s: cubic Hermite in physical time on the
//                      node positions and velocities (the state carries the velocity: C1, error h_n^4 / 384 max |p''''|), by
//                      trajectory_device.hpp's tr_state, as every later kernel of the chain places an object;
//   screen_kernel      for every (row, column) pair and every grid interval the closest approach of the two Hermite arcs -- chord
//                      minimum, then three Newton steps on d . d' -- reduced to one (distance, partner, time) per row and, with a
//                      threshold, to a list of the pairs that come closer than it;
//   pairs_kernel       the same closest approach for the pairs of a LIST (a screen's, flown again after a manoeuvre): one wave
//                      per pair, n x M work, the bits the screens give the pair;
//   events_kernel      EVERY close approach of the listed pairs: the local minima of the per-interval distance over the grid, one
//                      wave per pair, in the pairs-row form (i, j, distance, time) that the rest of the chain takes;
//   track_kernel       of those close approaches the one nearest each listed row's own time: an encounter followed through the
//                      re-screens of a manoeuvre, where pairs_kernel would jump to the pair's global minimum.
// Two screens launch screen_kernel.  All pairs of one constellation (SELF): rows and columns are the same S satellites, the full square of
// ordered pairs (i, j != i) is computed, the list holds the pairs i < j.  A constellation against a catalogue of foreign objects
// (cross): rows are the S satellites, columns the D objects, the rectangle S x D is computed and not the square (S + D)^2 of the
// union, the list holds every pair.
// One arithmetic for a pair whoever looks at it: the difference is always (higher index) - (lower index) in SELF, so (i, j) and
// (j, i) run the same operations on the same operands and get the same bits, and catalogue - satellite in cross, which is what
// SELF computes for the pair (i, S + j) of the union [constellation; catalogue], bit for bit.  Every reduction is a minimum under
// a total order (squared distance, then column index, then interval), so nothing depends on tiles, grid dimensions, row blocks
// or device count.
#include "mpcx_host.hpp"
#include "trajectory_device.hpp"

#include <math.h>

namespace mpcx {

constexpr int CJ_TC = 16;             // columns of a tile: a lane keeps the pair minimum of each in registers while it walks the grid
constexpr int CJ_MAXGROUPS = 64;      // all pairs: column groups (gridDim.y) at the most
constexpr int CJX_WAVES = 2048;       // cross: waves the launch aims at, two on each of the 256 x 4 SIMDs, what the kernel's registers admit
constexpr int CJX_WIDE_FROM = 512;    // cross: rows from which a workgroup takes 256 of them (four waves share the staged columns) instead of 64

// np.linspace(T0, T1, M)[m]: m * step, the last instant exactly T1 (a satellite whose span ends at T1 is still inside)
__device__ __forceinline__ double cj_time(int m, int M, double T0, double T1, double h)
{
    return m == M - 1 ? T1 : T0 + (double)m * h;
}

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
    for (int c = 0; c < 6; ++c) o[c] = cp_nan();
    const double t = cj_time(m, a.M, a.T0, a.T1, a.h);
    if (!bad && t >= ta && t <= tb) {
        const TrNode nd = tr_locate(nn, ta, tb, t);
        double h00, h10, h01, h11, p[3], v[3];
        tr_value_basis(nd.sg, h00, h10, h01, h11);
        const double L = a.units[2 * s], V = L / a.units[2 * s + 1];
        tr_state(a.Y + (size_t)s * 7 * a.n, (size_t)a.n, nd, h00, h10, h01, h11, L, V, p, v);
        for (int c = 0; c < 3; ++c) { o[c] = p[c]; o[3 + c] = v[c]; }
    }
    for (int c = 0; c < 6; ++c) a.eph[((size_t)s * 6 + c) * a.M + m] = o[c];
}

// eph [S][6][M] -> the screen's instant-major copy ephT [M][6][S] (the rows of one instant side by side: a row tile's loads
// are coalesced, an instant's S x 48 B stay in L2 across the row tiles).  An end with a NaN in any of its six values becomes
// NaN in all six, so that the screen tests positions only.  One lane per (instant, satellite).
__global__ __launch_bounds__(256) void conjunction_transpose_kernel(int S, int M, const double *eph, double *ephT)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)S * M) return;
    const int m = (int)(idx / S), s = (int)(idx - (long)m * S);
    double v[6];
    bool nan = false;
    for (int c = 0; c < 6; ++c) { v[c] = eph[((size_t)s * 6 + c) * M + m]; nan = nan || !(v[c] == v[c]); }
    for (int c = 0; c < 6; ++c) ephT[((size_t)m * 6 + c) * S + s] = nan ? cp_nan() : v[c];
}

// The closest approach of one pair inside one grid interval.  d0, d1: hi - lo position differences at the interval's ends;
// cv0, cv1 / v0, v1: the column's and the row's velocities there (their difference, hi - lo, is formed only where the Newton
// steps need it; up: the column is the higher index).  Distances are compared squared (the root is taken once, on the way out).  Updates
// (best, tbest) when the interval comes closer: ends first, the interior point (tr_chord_start, tr_newton) last, each only if
// strictly smaller.
__device__ __forceinline__ void cj_interval(const double (&d0)[3], const double (&d1)[3], const double *cv0, const double *cv1,
                                            const double (&v0)[3], const double (&v1)[3], bool up, double h, double t0, double t1,
                                            double &best, double &tbest)
{
    const double q0 = cp_dot(d0, d0), q1 = cp_dot(d1, d1);
    if (!(q0 == q0) || !(q1 == q1)) return;                       // an end outside a satellite's span
    double q = q0, tq = t0;
    if (q1 < q) { q = q1; tq = t1; }
    double s = tr_chord_start(d0, d1);
    if (s > 0.0 && s < 1.0) {
        double a0[3], a1[3];                                      // h w0, h w1
        for (int c = 0; c < 3; ++c) {
            a0[c] = h * (up ? cv0[c] - v0[c] : v0[c] - cv0[c]);
            a1[c] = h * (up ? cv1[c] - v1[c] : v1[c] - cv1[c]);
        }
        double qs;
        s = tr_newton(d0, d1, a0, a1, s, qs);
        if (qs < q) { q = qs; tq = t0 + s * h; }
    }
    if (q < best) { best = q; tbest = tq; }
}

struct ScreenArgs {
    int C, M, row0, nrows, max_pairs; // C columns; the launch's rows are row0 .. row0 + nrows - 1 of the caller's
    double T0, T1, h, thr;
    const double *rowT;               // instant-major ends of the launch's rows [M][6][rstride], its first row at index 0
    size_t rstride;
    const double *colT;               // instant-major ends of the columns [M][6][C]
    double *pd2, *pt;                 // partial row minima [gridDim.y][nrows]: squared distance, time
    int32_t *pj;                      //                                         column index
    double *pairs;                    // [max_pairs][4]
    unsigned long long *count;
};

// One lane per row, a workgroup of ROWS rows (blockIdx.x) that takes the column tiles blockIdx.y, blockIdx.y + gridDim.y, ...
// For one tile of CJ_TC columns a lane walks all grid intervals with the tile's pair minima in registers (the minimum of a PAIR
// over the whole grid is what the pairs list needs); its own ends come coalesced from rowT once per interval and serve the whole
// tile, the columns' ends are staged in LDS, TM intervals at a time, and read by every lane at the same address (a broadcast, no
// bank conflict).  A row's minimum needs no atomics.  SELF: the columns are the rows' own constellation and row r is column
// row0 + r -- that pair is skipped, the difference is (higher index) - (lower index), and the list takes a pair from its lower
// row only.  Otherwise the difference is column - row and every pair is listed.  ROWS and gridDim.y are the launch's choice
// (ScreenLaunch): 64-row workgroups are single waves, so that a few rows against many columns still put a wave with 64 live
// lanes on every SIMD.
template <int ROWS, int TM, bool SELF> __global__ __launch_bounds__(ROWS) void screen_kernel(ScreenArgs a)
{
    __shared__ double col[(TM + 1) * CJ_TC * 6];                 // [instant of the chunk][column][px py pz vx vy vz]
    const int lane = threadIdx.x;
    const int r = blockIdx.x * ROWS + lane;                      // row of the launch's block of rows
    const bool row_ok = r < a.nrows;
    const size_t ir = row_ok ? r : 0;                            // (lanes past the last row load the first row's ends and record nothing)
    const int i = a.row0 + (int)ir;                              // SELF: the row's index among the columns
    const size_t R = a.rstride, C = (size_t)a.C;
    double bd2 = cp_inf(), bt = cp_nan();
    int bj = -1;
    const int ntile = (a.C + CJ_TC - 1) / CJ_TC;
    for (int jt = blockIdx.y; jt < ntile; jt += gridDim.y) {
        const int j0 = jt * CJ_TC;
        double pd2[CJ_TC], pt[CJ_TC];
#pragma unroll
        for (int jj = 0; jj < CJ_TC; ++jj) { pd2[jj] = cp_inf(); pt[jj] = cp_nan(); }
        for (int m0 = 0; m0 < a.M - 1; m0 += TM) {
            const int nm = a.M - 1 - m0 < TM ? a.M - 1 - m0 : TM;                // intervals of this chunk
            __syncthreads();
            for (int e = lane; e < (nm + 1) * CJ_TC * 6; e += ROWS) {
                const int mm = e / (CJ_TC * 6), q = e - mm * (CJ_TC * 6), c = q / CJ_TC, jj = q - c * CJ_TC;
                const int j = j0 + jj;
                col[(mm * CJ_TC + jj) * 6 + c] = j < a.C ? a.colT[((size_t)(m0 + mm) * 6 + c) * C + j] : cp_nan();
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
                for (int jj = 0; jj < CJ_TC; ++jj) {
                    const int j = j0 + jj;
                    if ((SELF && j == i) || !row_ok) continue;
                    const double *c0 = col + (mm * CJ_TC + jj) * 6, *c1 = c0 + CJ_TC * 6;
                    const bool up = !SELF || j > i;                              // the column is the higher index: column - row
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
            if (!(pd2[jj] < cp_inf())) continue;                                 // no valid interval for this pair (or j == i, j >= C)
            if (pd2[jj] < bd2 || (pd2[jj] == bd2 && j < bj)) { bd2 = pd2[jj]; bt = pt[jj]; bj = j; }
            if (a.thr > 0.0 && (!SELF || j > i)) {
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

// the column groups' partial minima of every row -> dmin, partner, tca (a minimum under (distance, partner): any order gives it)
__global__ __launch_bounds__(256) void conjunction_reduce_kernel(int nrows, int ngroups, const double *pd2, const double *pt, const int32_t *pj,
                                                                 double *dmin, int32_t *partner, double *tca)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= nrows) return;
    double bd2 = cp_inf(), bt = cp_nan();
    int bj = -1;
    for (int g = 0; g < ngroups; ++g) {
        const size_t at = (size_t)g * nrows + r;
        const int j = pj[at];
        if (j < 0) continue;
        const double d2 = pd2[at];
        if (bj < 0 || d2 < bd2 || (d2 == bd2 && j < bj)) { bd2 = d2; bt = pt[at]; bj = j; }
    }
    dmin[r] = bj < 0 ? cp_inf() : sqrt(bd2);
    partner[r] = bj;
    tca[r] = bt;
}

struct PairsArgs {
    int n, S, D, M;                   // D = 0: j indexes the constellation as i does (all pairs); D > 0: the catalogue
    double T0, T1, h;
    const double *pairs;              // [n][4], columns 0 and 1 are read
    const double *eph, *cat;          // [S][6][M], [D][6][M] (cat = eph when D = 0)
    double *out;                      // [n][4]
    int32_t *status;                  // [n]
};

// an index column of the list -> the index, -1 where it is not a whole number of 0 .. N-1 (NaN and infinities among them)
__device__ __forceinline__ int cj_index(double x, int N) { return x >= 0.0 && x < (double)N && x == (double)(int)x ? (int)x : -1; }

// one object's end at instant m from its rows of eph [6][M]; a NaN in any of the six values is a NaN in all of them
// (conjunction_transpose_kernel's rule: the screen reads its ends behind it)
__device__ __forceinline__ void cj_end(const double *e, int M, int m, double (&p)[3], double (&v)[3])
{
    bool nan = false;
    for (int c = 0; c < 3; ++c) {
        p[c] = e[(size_t)c * M + m]; v[c] = e[(size_t)(3 + c) * M + m];
        nan = nan || !(p[c] == p[c]) || !(v[c] == v[c]);
    }
    for (int c = 0; c < 3; ++c) { p[c] = nan ? cp_nan() : p[c]; v[c] = nan ? cp_nan() : v[c]; }
}

// Grid interval m of a listed pair through cj_interval into (best, tbest).  er, ec: the rows of the ephemerides of object i (the
// row) and object j (the column); the row / column roles and `up` are screen_kernel's, so the interval's (q, t) are the screen's bits.
__device__ __forceinline__ void cj_pair_interval(const PairsArgs &a, const double *er, const double *ec, bool up, int m, double &best,
                                                 double &tbest)
{
    double p0[3], v0[3], p1[3], v1[3], c0[6], c1[6];
    {
        double cp[3], cv[3];
        cj_end(er, a.M, m, p0, v0); cj_end(er, a.M, m + 1, p1, v1);
        cj_end(ec, a.M, m, cp, cv);
        for (int c = 0; c < 3; ++c) { c0[c] = cp[c]; c0[3 + c] = cv[c]; }
        cj_end(ec, a.M, m + 1, cp, cv);
        for (int c = 0; c < 3; ++c) { c1[c] = cp[c]; c1[3 + c] = cv[c]; }
    }
    const double t0 = cj_time(m, a.M, a.T0, a.T1, a.h), t1 = cj_time(m + 1, a.M, a.T0, a.T1, a.h);
    double d0[3], d1[3];
    for (int c = 0; c < 3; ++c) {
        d0[c] = up ? c0[c] - p0[c] : p0[c] - c0[c];
        d1[c] = up ? c1[c] - p1[c] : p1[c] - c1[c];
    }
    cj_interval(d0, d1, c0 + 3, c1 + 3, v0, v1, up, a.h, t0, t1, best, tbest);
}

// The closest approach of LISTED pairs: n x M work where the screens do S^2 x M.  One wave per pair (blockIdx.x = the list's row);
// lane l takes the grid intervals l, l + 64, ... in ascending order through cj_interval, with the row / column roles and `up` as
// screen_kernel forms them (row = i, column = j; the difference is (higher index) - (lower index), against a catalogue column - row),
// so an interval's (q, t) are the screen's bits.  The screen keeps a pair's minimum over the intervals in ascending order, each only
// if strictly smaller: the smallest q, of equal ones the earliest interval.  Here every lane keeps (q, t, interval) of its own
// intervals under that rule and an xor butterfly takes the minimum under (q, interval) over the lanes -- a total order, so every
// lane ends with the same triple and the result does not depend on how the intervals were dealt out.  Lane 0 stores.
__global__ __launch_bounds__(64) void pairs_kernel(PairsArgs a)
{
    const int r = blockIdx.x, lane = threadIdx.x;
    const bool cross = a.D > 0;
    const double xi = a.pairs[(size_t)r * 4], xj = a.pairs[(size_t)r * 4 + 1];
    const int i = cj_index(xi, a.S), j = cj_index(xj, cross ? a.D : a.S);
    double *o = a.out + (size_t)r * 4;
    if (i < 0 || j < 0 || (!cross && i == j)) {                      // (the whole wave: it reads nothing of the ephemerides)
        if (lane == 0) { o[0] = xi; o[1] = xj; o[2] = cp_nan(); o[3] = cp_nan(); a.status[r] = MPCX_ST_BADK; }
        return;
    }
    const bool up = cross || j > i;                                  // the column is the higher index: column - row
    const double *er = a.eph + (size_t)i * 6 * a.M, *ec = (cross ? a.cat : a.eph) + (size_t)j * 6 * a.M;
    double best = cp_inf(), tbest = cp_nan();
    int mbest = 0x7fffffff;
    for (int m = lane; m < a.M - 1; m += 64) {
        const double before = best;
        cj_pair_interval(a, er, ec, up, m, best, tbest);
        if (best < before) mbest = m;
    }
    for (int w = 32; w >= 1; w >>= 1) {
        const double qo = __shfl_xor(best, w), to = __shfl_xor(tbest, w);
        const int mo = __shfl_xor(mbest, w);
        if (qo < best || (qo == best && mo < mbest)) { best = qo; tbest = to; mbest = mo; }
    }
    if (lane == 0) {
        o[0] = xi; o[1] = xj;
        o[2] = best < cp_inf() ? sqrt(best) : cp_inf();              // no valid interval: +inf, NaN, as the screens' rows have it
        o[3] = best < cp_inf() ? tbest : cp_nan();
        a.status[r] = MPCX_ST_OK;
    }
}

struct EventsArgs {
    PairsArgs p;                      // p.out: events [n][E][4]
    double thr;                       // metres; <= 0: every event
    int E;                            // slots per pair
    int32_t *info, *count;            // [n][E][2] = (interval, edge), [n]
};

// EVERY close approach of listed pairs (include/mpcx.h: mpcx_conjunction_events).  With (q_m, t_m) what cj_interval gives interval
// m alone (best = +inf; q_m = +inf where an end is invalid), interval m holds an event iff q_m < +inf, q_m < q_m-1 and q_m <= q_m+1,
// a neighbour that is absent or does not exist counting as +inf: the local minima of the per-interval distance, a minimum on a
// grid node (the same bits in both adjoining intervals) given to the earlier interval once.  One wave per pair as in pairs_kernel,
// but the wave walks the grid in chunks of 64 CONSECUTIVE intervals, lane l taking interval 64 c + l, so that the neighbours are the
// lanes beside it: q_m-1 comes from the lane below (lane 0: `carry`, the previous chunk's lane 63), q_m+1 from the lane above
// (lane 63: the next chunk's lane 0).  For that last one chunk c - 1 is decided after chunk c has been computed -- a one-chunk
// software pipeline with the pending (q, t) in four registers; the pass after the last chunk decides it against "absent", and the
// first pass decides a pending chunk that is all absent and so holds no event (no special case, and no peeled copy of the loop).  The
// threshold is applied to the events, sqrt(q) <= thr as the screens compare.  The event lanes of a chunk take consecutive slots
// behind the running count (a ballot and the population count of the lanes below) and store their own rows, so the events leave
// in ascending interval order and the first E of them are kept; the slots behind them are filled with (i, j, NaN, NaN), (-1, 0).
// No LDS, no atomics: nothing depends on anything but the pair.  Compiled for exactly six waves per SIMD, pairs_kernel's occupancy:
// left alone the compiler takes 87 VGPRs (five waves) and spills 12 SGPRs into the lanes of one of them, and with a minimum of six
// alone (__launch_bounds__(64, 6)) it spills to scratch; aimed at six it schedules for 80 VGPRs and needs neither
// (profiles/conjunction_events.txt).
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6, 6))) void events_kernel(EventsArgs e)
{
    const PairsArgs &a = e.p;
    const int r = blockIdx.x, lane = threadIdx.x;
    const bool cross = a.D > 0;
    const double xi = a.pairs[(size_t)r * 4], xj = a.pairs[(size_t)r * 4 + 1];
    const int i = cj_index(xi, a.S), j = cj_index(xj, cross ? a.D : a.S);
    double *ev = a.out + (size_t)r * e.E * 4;
    int32_t *inf = e.info + (size_t)r * e.E * 2;
    const bool bad = i < 0 || j < 0 || (!cross && i == j);           // (the whole wave: it reads nothing of the ephemerides)
    int found = 0;
    if (!bad) {
        const bool up = cross || j > i;                              // the column is the higher index: column - row
        const double *er = a.eph + (size_t)i * 6 * a.M, *ec = (cross ? a.cat : a.eph) + (size_t)j * 6 * a.M;
        const int nchunk = (a.M - 1 + 63) / 64;
        double qp = cp_inf(), tp = cp_nan();                         // the pending chunk's interval of this lane
        double carry = cp_inf();                                     // q of the interval before the pending chunk's first
        for (int c = 0; c <= nchunk; ++c) {
            const int m = 64 * c + lane;
            double q = cp_inf(), t = cp_nan();
            if (m < a.M - 1) cj_pair_interval(a, er, ec, up, m, q, t);
            const int mp = m - 64;
            double left = __shfl_up(qp, 1), right = __shfl_down(qp, 1);
            const double next = __shfl(q, 0);
            if (lane == 0) left = carry;
            if (lane == 63) right = next;
            const double d = sqrt(qp);
            const bool event = qp < cp_inf() && qp < left && qp <= right && (!(e.thr > 0.0) || d <= e.thr);
            const unsigned long long lanes = __ballot(event);
            const int slot = found + __popcll(lanes & ((1ULL << lane) - 1ULL));
            if (event && slot < e.E) {
                // still closing where the pair's common span ends: the time is an assigned end of the interval, so == is exact
                const bool edge = (!(left < cp_inf()) && tp == cj_time(mp, a.M, a.T0, a.T1, a.h)) ||
                                  (!(right < cp_inf()) && tp == cj_time(mp + 1, a.M, a.T0, a.T1, a.h));
                double *o = ev + (size_t)slot * 4;
                o[0] = xi; o[1] = xj; o[2] = d; o[3] = tp;
                inf[2 * slot] = mp; inf[2 * slot + 1] = edge ? 1 : 0;
            }
            found += __popcll(lanes);
            carry = __shfl(qp, 63);
            qp = q; tp = t;
        }
    }
    for (int s = (found < e.E ? found : e.E) + lane; s < e.E; s += 64) {
        double *o = ev + (size_t)s * 4;
        o[0] = xi; o[1] = xj; o[2] = cp_nan(); o[3] = cp_nan();
        inf[2 * s] = -1; inf[2 * s + 1] = 0;
    }
    if (lane == 0) { e.count[r] = found; a.status[r] = bad ? MPCX_ST_BADK : MPCX_ST_OK; }
}

struct TrackArgs {
    PairsArgs p;                      // p.pairs: column 3 is the time to follow; p.out: [n][4]
    double max_shift;                 // seconds; <= 0: unlimited
    int32_t *info;                    // [n][2] = (interval, edge), or NULL
};

// The close approach of a listed row that lies NEAREST THE ROW'S OWN TIME (include/mpcx.h: mpcx_conjunction_track): of the events
// events_kernel finds without a threshold, the one that minimises (|t_m - t_row|, m) -- a total order, so a tie goes to the earlier
// interval.  pairs_kernel follows a pair's global minimum, which after a manoeuvre is no longer the encounter the row was listed
// for when the pair has several; this follows the encounter.  One wave per row and events_kernel's walk: chunks of 64 consecutive
// intervals, the neighbours from the lanes beside and the chunk carry, chunk c - 1 decided after chunk c is computed.  The event
// predicate and the edge rule are restated here operation for operation on the same operands (events_kernel is left as it is: its
// registers are tuned), so an event has the bits events_kernel stores for it.  There is no threshold -- the caller needs the distance
// of an encounter that a manoeuvre has opened beyond any -- and so no square root per lane.  Every lane keeps the key of its best
// candidate, |dt| and the interval, in three registers; an xor butterfly takes the minimum under (|dt|, interval) after the last
// pass; then three lanes evaluate the winning interval and its two neighbours once more -- cj_pair_interval on the same operands,
// so the same bits -- for the event's (q, t) and its edge flag, and one lane takes the one root and stores.  (Carrying q, t and the
// edge flag of the candidate through the loop instead costs five more registers across cj_interval's Newton steps: at six waves per
// SIMD that build spilt four VGPRs to scratch, profiles/conjunction_track.txt.)  No LDS, no atomics: nothing depends on anything
// but the row.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6, 6))) void track_kernel(TrackArgs e)
{
    const PairsArgs &a = e.p;
    const int r = blockIdx.x, lane = threadIdx.x;
    const bool cross = a.D > 0;
    const double xi = a.pairs[(size_t)r * 4], xj = a.pairs[(size_t)r * 4 + 1], trow = a.pairs[(size_t)r * 4 + 3];
    const int i = cj_index(xi, a.S), j = cj_index(xj, cross ? a.D : a.S);
    double *o = a.out + (size_t)r * 4;
    // (the whole wave: it reads nothing of the ephemerides; trow - trow is 0 for a finite time and NaN otherwise)
    if (i < 0 || j < 0 || (!cross && i == j) || !(trow - trow == 0.0)) {
        if (lane == 0) {
            o[0] = xi; o[1] = xj; o[2] = cp_nan(); o[3] = cp_nan();
            if (e.info) { e.info[2 * (size_t)r] = -1; e.info[2 * (size_t)r + 1] = 0; }
            a.status[r] = MPCX_ST_BADK;
        }
        return;
    }
    const bool up = cross || j > i;                                  // the column is the higher index: column - row
    const double *er = a.eph + (size_t)i * 6 * a.M, *ec = (cross ? a.cat : a.eph) + (size_t)j * 6 * a.M;
    const int nchunk = (a.M - 1 + 63) / 64;
    double qp = cp_inf(), tp = cp_nan();                             // the pending chunk's interval of this lane
    double carry = cp_inf();                                         // q of the interval before the pending chunk's first
    double bdt = cp_inf();                                           // this lane's best candidate: |dt| and the interval
    int bm = 0x7fffffff;                                             //   (INT_MAX: none)
    for (int c = 0; c <= nchunk; ++c) {
        const int m = 64 * c + lane;
        double q = cp_inf(), t = cp_nan();
        if (m < a.M - 1) cj_pair_interval(a, er, ec, up, m, q, t);
        const int mp = m - 64;
        double left = __shfl_up(qp, 1), right = __shfl_down(qp, 1);
        const double next = __shfl(q, 0);
        if (lane == 0) left = carry;
        if (lane == 63) right = next;
        const bool event = qp < cp_inf() && qp < left && qp <= right;
        const double dt = fabs(tp - trow);
        // (a lane's intervals ascend, so its own ties keep the earlier; the comparison is the butterfly's all the same)
        if (event && (!(e.max_shift > 0.0) || dt <= e.max_shift) && (dt < bdt || (dt == bdt && mp < bm))) { bdt = dt; bm = mp; }
        carry = __shfl(qp, 63);
        qp = q; tp = t;
    }
    for (int w = 32; w >= 1; w >>= 1) {
        const double dto = __shfl_xor(bdt, w);
        const int mo = __shfl_xor(bm, w);
        if (dto < bdt || (dto == bdt && mo < bm)) { bdt = dto; bm = mo; }
    }
    // Every lane holds the winner.  Lanes 0, 1, 2 evaluate the intervals bm - 1, bm, bm + 1 once more: the event's (q, t) and its two
    // neighbours' q, from which lane 1 restates events_kernel's edge rule on the same operands.
    const bool have = bm != 0x7fffffff;
    const int mw = bm - 1 + lane;
    double q = cp_inf(), t = cp_nan();
    if (have && lane < 3 && mw >= 0 && mw < a.M - 1) cj_pair_interval(a, er, ec, up, mw, q, t);
    const double left = __shfl_up(q, 1), right = __shfl_down(q, 1);
    if (lane == 1) {
        // still closing where the pair's common span ends: the time is an assigned end of the interval, so == is exact
        const bool edge = have && ((!(left < cp_inf()) && t == cj_time(bm, a.M, a.T0, a.T1, a.h)) ||
                                   (!(right < cp_inf()) && t == cj_time(bm + 1, a.M, a.T0, a.T1, a.h)));
        o[0] = xi; o[1] = xj;
        o[2] = have ? sqrt(q) : cp_inf();                            // no event (within max_shift): +inf, NaN, as pairs_kernel's
        o[3] = have ? t : cp_nan();                                  // row without a valid interval
        if (e.info) { e.info[2 * (size_t)r] = have ? bm : -1; e.info[2 * (size_t)r + 1] = edge ? 1 : 0; }
        a.status[r] = MPCX_ST_OK;
    }
}

// The two screens as the host sees them: the name in the messages, and whether the columns are the rows' own constellation
// (then the callers below pass D = S and cat = eph).
struct Screen {
    const char *name;
    bool self;
};
constexpr Screen ALL_PAIRS{"conjunction_screen", true}, CROSS{"conjunction_cross_screen", false};

// The launch shape of nrows rows against C columns: rows per workgroup, row tiles (gridDim.x), column groups (gridDim.y, at most
// one per column tile).  All pairs: 256 rows always, enough groups for about four workgroups per compute unit whatever the number
// of row tiles, at most CJ_MAXGROUPS.  Cross: 256 rows from CJX_WIDE_FROM rows on and 64 below, and as many groups as it takes to
// reach CJX_WAVES waves.
struct ScreenLaunch {
    int rows, rowtiles, groups;
    ScreenLaunch(bool self, int nrows, int C)
    {
        rows = self || nrows >= CJX_WIDE_FROM ? 256 : 64;
        rowtiles = (nrows + rows - 1) / rows;
        const int waves = rowtiles * (rows / 64), ntile = (C + CJ_TC - 1) / CJ_TC;
        groups = self ? (1024 + rowtiles - 1) / rowtiles : (CJX_WAVES + waves - 1) / waves;
        if (groups > ntile) groups = ntile;
        if (self && groups > CJ_MAXGROUPS) groups = CJ_MAXGROUPS;
    }
};

static size_t cj_align(size_t b) { return (b + 255) & ~(size_t)255; }

// workspace: [rowT M*6*S][colT M*6*D][partial d2][partial t][partial j], and behind them, for the fused calls alone, [eph S*6*M]
// [cat D*6*M]: a _dev caller brings its ephemerides and does not pay for a second copy of them.  All pairs: the columns are the
// rows, colT = rowT and cat = eph take no room of their own.  The partial minima are groups * nrows entries: at most
// CJ_MAXGROUPS * S for all pairs; for cross at most (CJX_WAVES / waves + 1) * nrows with waves >= nrows / 64.
struct ScreenWorkspace {
    double *rowT, *colT, *pd2, *pt, *eph, *cat;
    int32_t *pj;
    size_t bytes;
    ScreenWorkspace(void *base, bool self, int S, int D, int M, bool fused)
    {
        char *p = (char *)base;
        const size_t e = cj_align((size_t)S * 6 * M * sizeof(double)), c = self ? 0 : cj_align((size_t)D * 6 * M * sizeof(double));
        const size_t g = cj_align((self ? (size_t)CJ_MAXGROUPS * S : (size_t)CJX_WAVES * 64 + (size_t)S + 256) * sizeof(double));
        rowT = colT = (double *)p; p += e;
        if (!self) { colT = (double *)p; p += c; }
        pd2 = (double *)p; p += g;
        pt = (double *)p; p += g;
        pj = (int32_t *)p; p += g;
        eph = cat = fused ? (double *)p : nullptr;
        if (fused) {
            p += e;
            if (!self) { cat = (double *)p; p += c; }
        }
        bytes = (size_t)(p - (char *)base);
    }
};

// what every screen entry point is given behind its ephemerides
struct ScreenCall {
    int S, D, M;
    double T0, T1;
    int row0, nrows;
    double threshold;
    int max_pairs;
    double *dmin;
    int32_t *partner;
    double *tca, *pairs;
    int64_t *n_pairs;
};

static int screen_fail(mpcx_ctx *ctx, const char *name, const char *what)
{
    char msg[200];
    snprintf(msg, sizeof msg, "%s: %s", name, what);
    return ctx_fail(ctx, MPCX_E_BADARG, msg);
}

static int screen_check(mpcx_ctx *ctx, const Screen &sc, const ScreenCall &c)
{
    if (c.S < 1 || c.D < 1 || c.M < 2 || !(c.T1 > c.T0) || c.max_pairs < 0)
        return screen_fail(ctx, sc.name, sc.self ? "need S>=1, M>=2, T1>T0, max_pairs>=0" : "need S>=1, D>=1, M>=2, T1>T0, max_pairs>=0");
    if (c.row0 < 0 || c.nrows < 1 || c.row0 > c.S - c.nrows) return screen_fail(ctx, sc.name, "rows row0 .. row0+nrows-1 must lie in 0 .. S-1");
    if (c.threshold > 0.0 && (!c.n_pairs || (c.max_pairs > 0 && !c.pairs)))
        return screen_fail(ctx, sc.name, "a threshold needs n_pairs, and pairs when max_pairs > 0");
    return MPCX_OK;
}

static int eph_check(mpcx_ctx *ctx, int S, int n, int M, double T0, double T1)
{
    if (S < 1 || M < 2 || n < 1 || !(T1 > T0)) return ctx_fail(ctx, MPCX_E_BADARG, "ephemeris: need S>=1, n>=1, M>=2, T1>T0");
    return MPCX_OK;
}

static unsigned cj_blocks(long lanes) { return (unsigned)((lanes + 255) / 256); }

// transpose -> memset -> screen -> reduce on `st`, everything in device memory (the two _dev entry points, checked by them)
static int screen_enqueue(mpcx_ctx *ctx, const Screen &sc, const ScreenCall &c, const double *eph, const double *cat, void *workspace,
                          hipStream_t st)
{
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    const ScreenWorkspace ws(workspace, sc.self, c.S, c.D, c.M, false);
    // all pairs: one copy of the whole constellation is rows and columns; cross: the launch's rows alone, and the whole catalogue
    const int trows = sc.self ? c.S : c.nrows;
    hipLaunchKernelGGL(conjunction_transpose_kernel, dim3(cj_blocks((long)trows * c.M)), dim3(256), 0, st, trows, c.M,
                       sc.self ? eph : eph + (size_t)c.row0 * 6 * c.M, ws.rowT);
    MPCX_HIP(ctx, hipGetLastError());
    if (!sc.self) {
        hipLaunchKernelGGL(conjunction_transpose_kernel, dim3(cj_blocks((long)c.D * c.M)), dim3(256), 0, st, c.D, c.M, cat, ws.colT);
        MPCX_HIP(ctx, hipGetLastError());
    }
    if (c.n_pairs) MPCX_HIP(ctx, hipMemsetAsync(c.n_pairs, 0, sizeof(int64_t), st));
    const ScreenLaunch L(sc.self, c.nrows, c.D);
    const ScreenArgs a{c.D, c.M, c.row0, c.nrows, c.max_pairs, c.T0, c.T1, (c.T1 - c.T0) / (double)(c.M - 1), c.threshold > 0.0 ? c.threshold : 0.0,
                       sc.self ? ws.rowT + c.row0 : ws.rowT, (size_t)trows, ws.colT, ws.pd2, ws.pt, ws.pj, c.pairs, (unsigned long long *)c.n_pairs};
    const dim3 grid((unsigned)L.rowtiles, (unsigned)L.groups);
    if (sc.self) hipLaunchKernelGGL((screen_kernel<256, 32, true>), grid, dim3(256), 0, st, a);
    else if (L.rows == 256) hipLaunchKernelGGL((screen_kernel<256, 32, false>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((screen_kernel<64, 16, false>), grid, dim3(64), 0, st, a);
    MPCX_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(conjunction_reduce_kernel, dim3(cj_blocks(c.nrows)), dim3(256), 0, st, c.nrows, L.groups, ws.pd2, ws.pt, ws.pj, c.dmin,
                       c.partner, c.tca);
    MPCX_HIP(ctx, hipGetLastError());
    return MPCX_OK;
}

// the part the four host-pointer screens share: the ephemerides already in HBM -> results in the caller's arrays
static int screen_from_device(mpcx_ctx *ctx, DeviceArena &ar, const Screen &sc, const ScreenCall &c, const double *deph, const double *dcat,
                              void *dws)
{
    ScreenCall d = c;
    d.dmin = ar.alloc<double>(c.nrows); d.tca = ar.alloc<double>(c.nrows);
    d.partner = ar.alloc<int32_t>(c.nrows);
    d.pairs = c.threshold > 0.0 && c.max_pairs > 0 ? ar.alloc<double>((size_t)c.max_pairs * 4) : nullptr;
    d.n_pairs = ar.alloc<int64_t>(1);
    if (ar.failed()) return ar.code();
    if (d.pairs) MPCX_HIP(ctx, hipMemsetAsync(d.pairs, 0, (size_t)c.max_pairs * 4 * sizeof(double), ctx->stream));
    if (int rc = screen_enqueue(ctx, sc, d, deph, dcat, dws, ctx->stream)) return rc;
    ar.download(c.dmin, d.dmin, c.nrows); ar.download(c.partner, d.partner, c.nrows); ar.download(c.tca, d.tca, c.nrows);
    if (d.pairs) ar.download(c.pairs, d.pairs, (size_t)c.max_pairs * 4);
    if (c.n_pairs) ar.download(c.n_pairs, d.n_pairs, 1);
    return ar.finish();
}

}  // namespace mpcx

using namespace mpcx;

extern "C" size_t mpcx_conjunction_workspace_bytes(int S, int M)
{
    if (S < 1 || M < 2) return 0;
    return ScreenWorkspace(nullptr, true, S, S, M, true).bytes;      // (with the fused call's ephemeris: the value callers have sized by)
}

extern "C" size_t mpcx_conjunction_cross_workspace_bytes(int S, int D, int M)
{
    if (S < 1 || D < 1 || M < 2) return 0;
    return ScreenWorkspace(nullptr, false, S, D, M, false).bytes;
}

extern "C" int mpcx_ephemeris_batch_dev(mpcx_ctx *ctx, int S, int n, const int32_t *ns, const double *Y, const double *units,
                                        const double *span, int M, double T0, double T1, double *eph, int32_t *status, void *stream)
{
    if (!ctx) return MPCX_E_BADARG;
    if (int rc = eph_check(ctx, S, n, M, T0, T1)) return rc;
    if (!Y || !units || !span || !eph || !status) return ctx_fail(ctx, MPCX_E_BADARG, "ephemeris: Y, units, span, eph and status are required");
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    EphArgs a{S, n, M, ns, Y, units, span, T0, T1, (T1 - T0) / (double)(M - 1), eph, status};
    hipLaunchKernelGGL(ephemeris_kernel, dim3(cj_blocks((long)S * M)), dim3(256), 0, (hipStream_t)stream, a);
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

extern "C" int mpcx_conjunction_screen_dev(mpcx_ctx *ctx, int S, int M, const double *eph, double T0, double T1, int row0, int nrows,
                                           double threshold, int max_pairs, double *dmin, int32_t *partner, double *tca, double *pairs,
                                           int64_t *n_pairs, void *workspace, void *stream)
{
    if (!ctx) return MPCX_E_BADARG;
    const ScreenCall c{S, S, M, T0, T1, row0, nrows, threshold, max_pairs, dmin, partner, tca, pairs, n_pairs};
    if (int rc = screen_check(ctx, ALL_PAIRS, c)) return rc;
    if (!eph || !dmin || !partner || !tca || !workspace) return screen_fail(ctx, ALL_PAIRS.name, "eph, dmin, partner, tca and workspace are required");
    return screen_enqueue(ctx, ALL_PAIRS, c, eph, eph, workspace, (hipStream_t)stream);
}

extern "C" int mpcx_conjunction_cross_screen_dev(mpcx_ctx *ctx, int S, int D, int M, const double *eph, const double *cat, double T0,
                                                 double T1, int row0, int nrows, double threshold, int max_pairs, double *dmin,
                                                 int32_t *partner, double *tca, double *pairs, int64_t *n_pairs, void *workspace,
                                                 void *stream)
{
    if (!ctx) return MPCX_E_BADARG;
    const ScreenCall c{S, D, M, T0, T1, row0, nrows, threshold, max_pairs, dmin, partner, tca, pairs, n_pairs};
    if (int rc = screen_check(ctx, CROSS, c)) return rc;
    if (!eph || !cat || !dmin || !partner || !tca || !workspace)
        return screen_fail(ctx, CROSS.name, "eph, cat, dmin, partner, tca and workspace are required");
    return screen_enqueue(ctx, CROSS, c, eph, cat, workspace, (hipStream_t)stream);
}

extern "C" int mpcx_conjunction_screen(mpcx_ctx *ctx, int S, int M, const double *eph, double T0, double T1, int row0, int nrows,
                                       double threshold, int max_pairs, double *dmin, int32_t *partner, double *tca, double *pairs,
                                       int64_t *n_pairs)
{
    if (!ctx) return MPCX_E_BADARG;
    const ScreenCall c{S, S, M, T0, T1, row0, nrows, threshold, max_pairs, dmin, partner, tca, pairs, n_pairs};
    if (int rc = screen_check(ctx, ALL_PAIRS, c)) return rc;
    if (!eph || !dmin || !partner || !tca) return screen_fail(ctx, ALL_PAIRS.name, "eph, dmin, partner and tca are required");
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    DeviceArena ar(ctx);
    double *de = ar.upload(eph, (size_t)S * 6 * M);
    char *dws = ar.alloc<char>(mpcx_conjunction_workspace_bytes(S, M));
    if (ar.failed()) return ar.code();
    return screen_from_device(ctx, ar, ALL_PAIRS, c, de, de, dws);
}

extern "C" int mpcx_conjunction_cross_screen(mpcx_ctx *ctx, int S, int D, int M, const double *eph, const double *cat, double T0, double T1,
                                             int row0, int nrows, double threshold, int max_pairs, double *dmin, int32_t *partner,
                                             double *tca, double *pairs, int64_t *n_pairs)
{
    if (!ctx) return MPCX_E_BADARG;
    const ScreenCall c{S, D, M, T0, T1, row0, nrows, threshold, max_pairs, dmin, partner, tca, pairs, n_pairs};
    if (int rc = screen_check(ctx, CROSS, c)) return rc;
    if (!eph || !cat || !dmin || !partner || !tca) return screen_fail(ctx, CROSS.name, "eph, cat, dmin, partner and tca are required");
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    DeviceArena ar(ctx);
    double *de = ar.upload(eph, (size_t)S * 6 * M), *dc = ar.upload(cat, (size_t)D * 6 * M);
    char *dws = ar.alloc<char>(mpcx_conjunction_cross_workspace_bytes(S, D, M));
    if (ar.failed()) return ar.code();
    return screen_from_device(ctx, ar, CROSS, c, de, dc, dws);
}

extern "C" int mpcx_conjunction_screen_traj(mpcx_ctx *ctx, int S, int n, const int32_t *ns, const double *Y, const double *units,
                                            const double *span, int M, double T0, double T1, int row0, int nrows, double threshold,
                                            int max_pairs, double *dmin, int32_t *partner, double *tca, double *pairs, int64_t *n_pairs,
                                            int32_t *status)
{
    if (!ctx) return MPCX_E_BADARG;
    const ScreenCall c{S, S, M, T0, T1, row0, nrows, threshold, max_pairs, dmin, partner, tca, pairs, n_pairs};
    if (int rc = eph_check(ctx, S, n, M, T0, T1)) return rc;
    if (int rc = screen_check(ctx, ALL_PAIRS, c)) return rc;
    if (!Y || !units || !span || !dmin || !partner || !tca)
        return screen_fail(ctx, "conjunction_screen_traj", "Y, units, span, dmin, partner and tca are required");
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    DeviceArena ar(ctx);
    double *dY = ar.upload(Y, (size_t)S * 7 * n), *du = ar.upload(units, (size_t)S * 2), *dsp = ar.upload(span, (size_t)S * 2);
    int32_t *dns = ns ? ar.upload(ns, S) : nullptr;
    int32_t *dst = ar.alloc<int32_t>(S);
    char *dws = ar.alloc<char>(mpcx_conjunction_workspace_bytes(S, M));
    if (ar.failed()) return ar.code();
    const ScreenWorkspace ws(dws, true, S, S, M, true);              // the ephemeris never leaves HBM
    if (int rc = mpcx_ephemeris_batch_dev(ctx, S, n, dns, dY, du, dsp, M, T0, T1, ws.eph, dst, ctx->stream)) return rc;
    if (status) ar.download(status, dst, S);
    return screen_from_device(ctx, ar, ALL_PAIRS, c, ws.eph, ws.eph, dws);
}

extern "C" int mpcx_conjunction_cross_screen_traj(mpcx_ctx *ctx, int S, int n, const int32_t *ns, const double *Y, const double *units,
                                                  const double *span, int D, int cat_n, const int32_t *cat_ns, const double *cat_Y,
                                                  const double *cat_units, const double *cat_span, int M, double T0, double T1, int row0,
                                                  int nrows, double threshold, int max_pairs, double *dmin, int32_t *partner, double *tca,
                                                  double *pairs, int64_t *n_pairs, int32_t *status, int32_t *cat_status)
{
    if (!ctx) return MPCX_E_BADARG;
    const ScreenCall c{S, D, M, T0, T1, row0, nrows, threshold, max_pairs, dmin, partner, tca, pairs, n_pairs};
    if (S < 1 || D < 1 || M < 2 || n < 1 || cat_n < 1 || !(T1 > T0))
        return screen_fail(ctx, "conjunction_cross_screen_traj", "need S>=1, D>=1, n>=1, cat_n>=1, M>=2, T1>T0");
    if (int rc = screen_check(ctx, CROSS, c)) return rc;
    if (!Y || !units || !span || !cat_Y || !cat_units || !cat_span || !dmin || !partner || !tca)
        return screen_fail(ctx, "conjunction_cross_screen_traj", "Y, units, span, cat_Y, cat_units, cat_span, dmin, partner and tca are required");
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    DeviceArena ar(ctx);
    double *dY = ar.upload(Y, (size_t)S * 7 * n), *du = ar.upload(units, (size_t)S * 2), *dsp = ar.upload(span, (size_t)S * 2);
    int32_t *dns = ns ? ar.upload(ns, S) : nullptr;
    double *cY = ar.upload(cat_Y, (size_t)D * 7 * cat_n), *cu = ar.upload(cat_units, (size_t)D * 2), *csp = ar.upload(cat_span, (size_t)D * 2);
    int32_t *cns = cat_ns ? ar.upload(cat_ns, D) : nullptr;
    int32_t *dst = ar.alloc<int32_t>(S), *cst = ar.alloc<int32_t>(D);
    char *dws = ar.alloc<char>(ScreenWorkspace(nullptr, false, S, D, M, true).bytes);   // the screen's workspace, then the two ephemerides
    if (ar.failed()) return ar.code();
    const ScreenWorkspace ws(dws, false, S, D, M, true);            // neither ephemeris leaves HBM
    if (int rc = mpcx_ephemeris_batch_dev(ctx, S, n, dns, dY, du, dsp, M, T0, T1, ws.eph, dst, ctx->stream)) return rc;
    if (int rc = mpcx_ephemeris_batch_dev(ctx, D, cat_n, cns, cY, cu, csp, M, T0, T1, ws.cat, cst, ctx->stream)) return rc;
    if (status) ar.download(status, dst, S);
    if (cat_status) ar.download(cat_status, cst, D);
    return screen_from_device(ctx, ar, CROSS, c, ws.eph, ws.cat, dws);
}

// ---- listed pairs: the closest approach of each (mpcx_conjunction_pairs*), every close approach (mpcx_conjunction_events*), or
// the close approach nearest each row's own time (mpcx_conjunction_track*)
namespace mpcx {

// what every list entry point is given behind its list and its two sides; events: every close approach below the threshold
// (events_kernel, max_events slots per pair) instead of the closest one (pairs_kernel); track: the close approach nearest the row's
// time, at most max_shift away (track_kernel)
struct PairsCall {
    int n, S, D, M;
    double T0, T1;
    bool events;
    double threshold;
    int max_events;
    bool track = false;
    double max_shift = 0.0;
    size_t rows() const { return (size_t)n * (events ? (size_t)max_events : 1); }       // rows of four doubles in the first output
};

// the outputs: rows = out [n][4] and status [n]; the events calls have rows = events [n][E][4], info [n][E][2] and count [n] too;
// the track calls may have info [n][2]
struct PairsOut {
    double *rows;
    int32_t *status, *info, *count;
    bool complete(const PairsCall &c) const { return rows && status && (!c.events || (info && count)); }
};

// the names in the messages
struct PairsNames {
    const char *call, *traj, *outs, *outs_list;
};
constexpr PairsNames PAIRS{"conjunction_pairs", "conjunction_pairs_traj", "out and status", "out, status"};
constexpr PairsNames EVENTS{"conjunction_events", "conjunction_events_traj", "events, info, count and status", "events, info, count, status"};
constexpr PairsNames TRACK{"conjunction_track", "conjunction_track_traj", "out and status", "out, status"};

static int pairs_check(mpcx_ctx *ctx, const char *name, const PairsCall &c)
{
    if (!c.events && !c.track && c.n < 1) return screen_fail(ctx, name, "need n>=1, S>=1, D>=0, M>=2, T1>T0");
    if (c.n < 0 || c.S < 1 || c.D < 0 || c.M < 2 || !(c.T1 > c.T0)) return screen_fail(ctx, name, "need n>=0, S>=1, D>=0, M>=2, T1>T0");
    if (c.events && (c.max_events < 1 || !(c.threshold == c.threshold)))
        return screen_fail(ctx, name, "need max_events>=1 and a threshold that is not NaN");
    if (c.track && !(c.max_shift == c.max_shift)) return screen_fail(ctx, name, "need a max_shift that is not NaN");
    return MPCX_OK;
}

static int pairs_missing(mpcx_ctx *ctx, const char *name, const char *fmt, const char *outs)
{
    char what[160];
    snprintf(what, sizeof what, fmt, outs);
    return screen_fail(ctx, name, what);
}

// the two ephemerides of the _traj calls: [eph S*6*M][cat D*6*M]
struct PairsWorkspace {
    double *eph, *cat;
    size_t bytes;
    PairsWorkspace(void *base, int S, int D, int M)
    {
        char *p = (char *)base;
        eph = (double *)p; p += cj_align((size_t)S * 6 * M * sizeof(double));
        cat = D > 0 ? (double *)p : eph;
        if (D > 0) p += cj_align((size_t)D * 6 * M * sizeof(double));
        bytes = (size_t)(p - (char *)base);
    }
};

// pairs_kernel, events_kernel or track_kernel on `st`, everything in device memory
static int pairs_enqueue(mpcx_ctx *ctx, const PairsCall &c, const double *pairs, const double *eph, const double *cat, const PairsOut &o,
                         hipStream_t st)
{
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    const PairsArgs a{c.n, c.S, c.D, c.M, c.T0, c.T1, (c.T1 - c.T0) / (double)(c.M - 1), pairs, eph, c.D > 0 ? cat : eph, o.rows, o.status};
    if (c.events) {
        const EventsArgs e{a, c.threshold > 0.0 ? c.threshold : 0.0, c.max_events, o.info, o.count};
        hipLaunchKernelGGL(events_kernel, dim3((unsigned)c.n), dim3(64), 0, st, e);
    } else if (c.track) {
        const TrackArgs t{a, c.max_shift > 0.0 ? c.max_shift : 0.0, o.info};
        hipLaunchKernelGGL(track_kernel, dim3((unsigned)c.n), dim3(64), 0, st, t);
    } else
        hipLaunchKernelGGL(pairs_kernel, dim3((unsigned)c.n), dim3(64), 0, st, a);
    MPCX_HIP(ctx, hipGetLastError());
    return MPCX_OK;
}

// device arrays for the outputs `o` of a host-pointer call, on their way back (a track call's info only where it is asked for)
static PairsOut pairs_results(DeviceArena &ar, const PairsCall &c, const PairsOut &o)
{
    PairsOut d{ar.result(o.rows, c.rows() * 4), ar.result(o.status, (size_t)c.n), nullptr, nullptr};
    if (c.events || c.track) d.info = ar.result(o.info, c.rows() * 2);
    if (c.events) d.count = ar.result(o.count, (size_t)c.n);
    return d;
}

// the four forms of a list call behind their extern "C" names (n = 0 passes pairs_check for the events and track calls only: nothing to do)
static int pairs_dev(mpcx_ctx *ctx, const PairsNames &nm, const PairsCall &c, const double *pairs, const double *eph, const double *cat,
                     const PairsOut &o, void *stream)
{
    if (int rc = pairs_check(ctx, nm.call, c)) return rc;
    if (c.n == 0) return MPCX_OK;
    if (!pairs || !eph || !o.complete(c) || (c.D > 0) != (cat != nullptr))
        return pairs_missing(ctx, nm.call, "pairs, eph, %s are required, and cat exactly when D > 0", nm.outs);
    return pairs_enqueue(ctx, c, pairs, eph, cat, o, (hipStream_t)stream);
}

static int pairs_host(mpcx_ctx *ctx, const PairsNames &nm, const PairsCall &c, const double *pairs, const double *eph, const double *cat,
                      const PairsOut &o)
{
    if (int rc = pairs_check(ctx, nm.call, c)) return rc;
    if (c.n == 0) return MPCX_OK;
    if (!pairs || !eph || !o.complete(c) || (c.D > 0) != (cat != nullptr))
        return pairs_missing(ctx, nm.call, "pairs, eph, %s are required, and cat exactly when D > 0", nm.outs);
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    DeviceArena ar(ctx);
    double *dp = ar.upload(pairs, (size_t)c.n * 4), *de = ar.upload(eph, (size_t)c.S * 6 * c.M);
    double *dc = c.D > 0 ? ar.upload(cat, (size_t)c.D * 6 * c.M) : nullptr;
    const PairsOut d = pairs_results(ar, c, o);
    return host_run(ctx, ar, 0, [&](void *, hipStream_t st) { return pairs_enqueue(ctx, c, dp, de, dc, d, st); });
}

// one side's trajectories as mpcx_ephemeris_batch takes them
struct PairsSide {
    int n;
    const int32_t *ns;
    const double *Y, *units, *span;
};

static int pairs_traj_dev(mpcx_ctx *ctx, const PairsNames &nm, const PairsCall &c, const double *pairs, const PairsSide &sat,
                          const PairsSide &cat, const PairsOut &o, int32_t *eph_status, int32_t *cat_status, void *workspace, void *stream)
{
    if (int rc = pairs_check(ctx, nm.traj, c)) return rc;
    if (c.n == 0) return MPCX_OK;
    if (sat.n < 1 || (c.D > 0 && cat.n < 1)) return screen_fail(ctx, nm.traj, "need n>=1 nodes on each side");
    if (!pairs || !sat.Y || !sat.units || !sat.span || !o.complete(c) || !eph_status || !workspace)
        return pairs_missing(ctx, nm.traj, "pairs, Y, units, span, %s, eph_status and workspace are required", nm.outs_list);
    if (c.D > 0 ? !cat.Y || !cat.units || !cat.span || !cat_status : cat.Y != nullptr)
        return screen_fail(ctx, nm.traj, "cat_Y, cat_units, cat_span and cat_status are required exactly when D > 0");
    const PairsWorkspace ws(workspace, c.S, c.D, c.M);
    if (int rc = mpcx_ephemeris_batch_dev(ctx, c.S, sat.n, sat.ns, sat.Y, sat.units, sat.span, c.M, c.T0, c.T1, ws.eph, eph_status, stream)) return rc;
    if (c.D > 0)
        if (int rc = mpcx_ephemeris_batch_dev(ctx, c.D, cat.n, cat.ns, cat.Y, cat.units, cat.span, c.M, c.T0, c.T1, ws.cat, cat_status, stream))
            return rc;
    return pairs_enqueue(ctx, c, pairs, ws.eph, ws.cat, o, (hipStream_t)stream);
}

static int pairs_traj_host(mpcx_ctx *ctx, const PairsNames &nm, const PairsCall &c, const double *pairs, const PairsSide &sat,
                           const PairsSide &cat, const PairsOut &o, int32_t *eph_status, int32_t *cat_status)
{
    if (int rc = pairs_check(ctx, nm.traj, c)) return rc;
    if (c.n == 0) return MPCX_OK;
    if (sat.n < 1 || (c.D > 0 && cat.n < 1)) return screen_fail(ctx, nm.traj, "need n>=1 nodes on each side");
    if (!pairs || !sat.Y || !sat.units || !sat.span || !o.complete(c))
        return pairs_missing(ctx, nm.traj, "pairs, Y, units, span, %s are required", nm.outs);
    if (c.D > 0 ? !cat.Y || !cat.units || !cat.span : cat.Y != nullptr)
        return screen_fail(ctx, nm.traj, "cat_Y, cat_units and cat_span are required exactly when D > 0");
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    DeviceArena ar(ctx);
    const int S = c.S, D = c.D;
    double *dp = ar.upload(pairs, (size_t)c.n * 4);
    PairsSide ds{sat.n, sat.ns ? ar.upload(sat.ns, S) : nullptr, ar.upload(sat.Y, (size_t)S * 7 * sat.n), ar.upload(sat.units, (size_t)S * 2),
                 ar.upload(sat.span, (size_t)S * 2)};
    PairsSide dc{cat.n, nullptr, nullptr, nullptr, nullptr};
    int32_t *cst = nullptr;
    if (D > 0) {
        dc = PairsSide{cat.n, cat.ns ? ar.upload(cat.ns, D) : nullptr, ar.upload(cat.Y, (size_t)D * 7 * cat.n), ar.upload(cat.units, (size_t)D * 2),
                       ar.upload(cat.span, (size_t)D * 2)};
        cst = ar.alloc<int32_t>(D);
    }
    int32_t *est = ar.alloc<int32_t>(S);
    const PairsOut d = pairs_results(ar, c, o);
    char *dws = ar.alloc<char>(PairsWorkspace(nullptr, S, D, c.M).bytes);                // neither ephemeris leaves HBM
    if (ar.failed()) return ar.code();
    if (int rc = pairs_traj_dev(ctx, nm, c, dp, ds, dc, d, est, cst, dws, ctx->stream)) return rc;
    ar.fetch();
    if (eph_status) ar.download(eph_status, est, S);
    if (D > 0 && cat_status) ar.download(cat_status, cst, D);
    return ar.finish();
}

}  // namespace mpcx

extern "C" size_t mpcx_conjunction_pairs_workspace_bytes(int S, int D, int M)
{
    if (S < 1 || D < 0 || M < 2) return 0;
    return PairsWorkspace(nullptr, S, D, M).bytes;
}

extern "C" int mpcx_conjunction_pairs_dev(mpcx_ctx *ctx, int n, const double *pairs, int S, int D, int M, const double *eph,
                                          const double *cat, double T0, double T1, double *out, int32_t *status, void *stream)
{
    if (!ctx) return MPCX_E_BADARG;
    return pairs_dev(ctx, PAIRS, PairsCall{n, S, D, M, T0, T1, false, 0.0, 0}, pairs, eph, cat, PairsOut{out, status, nullptr, nullptr}, stream);
}

extern "C" int mpcx_conjunction_pairs(mpcx_ctx *ctx, int n, const double *pairs, int S, int D, int M, const double *eph, const double *cat,
                                      double T0, double T1, double *out, int32_t *status)
{
    if (!ctx) return MPCX_E_BADARG;
    return pairs_host(ctx, PAIRS, PairsCall{n, S, D, M, T0, T1, false, 0.0, 0}, pairs, eph, cat, PairsOut{out, status, nullptr, nullptr});
}

extern "C" int mpcx_conjunction_pairs_traj_dev(mpcx_ctx *ctx, int n, const double *pairs, int S, int nn, const int32_t *ns, const double *Y,
                                               const double *units, const double *span, int D, int cat_n, const int32_t *cat_ns,
                                               const double *cat_Y, const double *cat_units, const double *cat_span, int M, double T0,
                                               double T1, double *out, int32_t *status, int32_t *eph_status, int32_t *cat_status,
                                               void *workspace, void *stream)
{
    if (!ctx) return MPCX_E_BADARG;
    return pairs_traj_dev(ctx, PAIRS, PairsCall{n, S, D, M, T0, T1, false, 0.0, 0}, pairs, PairsSide{nn, ns, Y, units, span},
                          PairsSide{cat_n, cat_ns, cat_Y, cat_units, cat_span}, PairsOut{out, status, nullptr, nullptr}, eph_status, cat_status,
                          workspace, stream);
}

extern "C" int mpcx_conjunction_pairs_traj(mpcx_ctx *ctx, int n, const double *pairs, int S, int nn, const int32_t *ns, const double *Y,
                                           const double *units, const double *span, int D, int cat_n, const int32_t *cat_ns,
                                           const double *cat_Y, const double *cat_units, const double *cat_span, int M, double T0, double T1,
                                           double *out, int32_t *status, int32_t *eph_status, int32_t *cat_status)
{
    if (!ctx) return MPCX_E_BADARG;
    return pairs_traj_host(ctx, PAIRS, PairsCall{n, S, D, M, T0, T1, false, 0.0, 0}, pairs, PairsSide{nn, ns, Y, units, span},
                           PairsSide{cat_n, cat_ns, cat_Y, cat_units, cat_span}, PairsOut{out, status, nullptr, nullptr}, eph_status, cat_status);
}

// ---- every close approach of the listed pairs: the same four forms on events_kernel.  An empty list (n = 0) is a successful call
// that does nothing: a screen that lists no pair is no error

extern "C" size_t mpcx_conjunction_events_workspace_bytes(int S, int D, int M) { return mpcx_conjunction_pairs_workspace_bytes(S, D, M); }

extern "C" int mpcx_conjunction_events_dev(mpcx_ctx *ctx, int n, const double *pairs, int S, int D, int M, const double *eph,
                                           const double *cat, double T0, double T1, double threshold, int max_events, double *events,
                                           int32_t *info, int32_t *count, int32_t *status, void *stream)
{
    if (!ctx) return MPCX_E_BADARG;
    return pairs_dev(ctx, EVENTS, PairsCall{n, S, D, M, T0, T1, true, threshold, max_events}, pairs, eph, cat, PairsOut{events, status, info, count},
                     stream);
}

extern "C" int mpcx_conjunction_events(mpcx_ctx *ctx, int n, const double *pairs, int S, int D, int M, const double *eph, const double *cat,
                                       double T0, double T1, double threshold, int max_events, double *events, int32_t *info,
                                       int32_t *count, int32_t *status)
{
    if (!ctx) return MPCX_E_BADARG;
    return pairs_host(ctx, EVENTS, PairsCall{n, S, D, M, T0, T1, true, threshold, max_events}, pairs, eph, cat, PairsOut{events, status, info, count});
}

extern "C" int mpcx_conjunction_events_traj_dev(mpcx_ctx *ctx, int n, const double *pairs, int S, int nn, const int32_t *ns, const double *Y,
                                                const double *units, const double *span, int D, int cat_n, const int32_t *cat_ns,
                                                const double *cat_Y, const double *cat_units, const double *cat_span, int M, double T0,
                                                double T1, double threshold, int max_events, double *events, int32_t *info, int32_t *count,
                                                int32_t *status, int32_t *eph_status, int32_t *cat_status, void *workspace, void *stream)
{
    if (!ctx) return MPCX_E_BADARG;
    return pairs_traj_dev(ctx, EVENTS, PairsCall{n, S, D, M, T0, T1, true, threshold, max_events}, pairs, PairsSide{nn, ns, Y, units, span},
                          PairsSide{cat_n, cat_ns, cat_Y, cat_units, cat_span}, PairsOut{events, status, info, count}, eph_status, cat_status,
                          workspace, stream);
}

extern "C" int mpcx_conjunction_events_traj(mpcx_ctx *ctx, int n, const double *pairs, int S, int nn, const int32_t *ns, const double *Y,
                                            const double *units, const double *span, int D, int cat_n, const int32_t *cat_ns,
                                            const double *cat_Y, const double *cat_units, const double *cat_span, int M, double T0, double T1,
                                            double threshold, int max_events, double *events, int32_t *info, int32_t *count,
                                            int32_t *status, int32_t *eph_status, int32_t *cat_status)
{
    if (!ctx) return MPCX_E_BADARG;
    return pairs_traj_host(ctx, EVENTS, PairsCall{n, S, D, M, T0, T1, true, threshold, max_events}, pairs, PairsSide{nn, ns, Y, units, span},
                           PairsSide{cat_n, cat_ns, cat_Y, cat_units, cat_span}, PairsOut{events, status, info, count}, eph_status, cat_status);
}

// ---- the close approach nearest each row's own time: the same four forms on track_kernel; n = 0 does nothing, info may be NULL

extern "C" size_t mpcx_conjunction_track_workspace_bytes(int S, int D, int M) { return mpcx_conjunction_pairs_workspace_bytes(S, D, M); }

extern "C" int mpcx_conjunction_track_dev(mpcx_ctx *ctx, int n, const double *pairs, int S, int D, int M, const double *eph,
                                          const double *cat, double T0, double T1, double max_shift, double *out, int32_t *info,
                                          int32_t *status, void *stream)
{
    if (!ctx) return MPCX_E_BADARG;
    return pairs_dev(ctx, TRACK, PairsCall{n, S, D, M, T0, T1, false, 0.0, 0, true, max_shift}, pairs, eph, cat, PairsOut{out, status, info, nullptr},
                     stream);
}

extern "C" int mpcx_conjunction_track(mpcx_ctx *ctx, int n, const double *pairs, int S, int D, int M, const double *eph, const double *cat,
                                      double T0, double T1, double max_shift, double *out, int32_t *info, int32_t *status)
{
    if (!ctx) return MPCX_E_BADARG;
    return pairs_host(ctx, TRACK, PairsCall{n, S, D, M, T0, T1, false, 0.0, 0, true, max_shift}, pairs, eph, cat, PairsOut{out, status, info, nullptr});
}

extern "C" int mpcx_conjunction_track_traj_dev(mpcx_ctx *ctx, int n, const double *pairs, int S, int nn, const int32_t *ns, const double *Y,
                                               const double *units, const double *span, int D, int cat_n, const int32_t *cat_ns,
                                               const double *cat_Y, const double *cat_units, const double *cat_span, int M, double T0,
                                               double T1, double max_shift, double *out, int32_t *info, int32_t *status, int32_t *eph_status,
                                               int32_t *cat_status, void *workspace, void *stream)
{
    if (!ctx) return MPCX_E_BADARG;
    return pairs_traj_dev(ctx, TRACK, PairsCall{n, S, D, M, T0, T1, false, 0.0, 0, true, max_shift}, pairs, PairsSide{nn, ns, Y, units, span},
                          PairsSide{cat_n, cat_ns, cat_Y, cat_units, cat_span}, PairsOut{out, status, info, nullptr}, eph_status, cat_status,
                          workspace, stream);
}

extern "C" int mpcx_conjunction_track_traj(mpcx_ctx *ctx, int n, const double *pairs, int S, int nn, const int32_t *ns, const double *Y,
                                           const double *units, const double *span, int D, int cat_n, const int32_t *cat_ns,
                                           const double *cat_Y, const double *cat_units, const double *cat_span, int M, double T0, double T1,
                                           double max_shift, double *out, int32_t *info, int32_t *status, int32_t *eph_status,
                                           int32_t *cat_status)
{
    if (!ctx) return MPCX_E_BADARG;
    return pairs_traj_host(ctx, TRACK, PairsCall{n, S, D, M, T0, T1, false, 0.0, 0, true, max_shift}, pairs, PairsSide{nn, ns, Y, units, span},
                           PairsSide{cat_n, cat_ns, cat_Y, cat_units, cat_span}, PairsOut{out, status, info, nullptr}, eph_status, cat_status);
}
