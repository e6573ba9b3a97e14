// collision_mc.hip -- the collision probability of listed pairs by sampled flights through the truth model (include/mpcx.h:
// mpcx_collision_probability_mc*).  Nothing here is linearised: initial states, masses and thrust execution errors are drawn, every
// draw is flown by propagate_kernel, and what is reported is how often two flown objects come within the summed radii.
//   mc_rows_kernel        once per call: every row's tests (cw_row's on the given trajectories, the flights' tf, both factors, the
//                         exec rows and mass variances) -> the window, R and the row's status.  One lane per row.
//   per chunk of samples (the chunking bounds the workspace and changes no bit):
//   mc_sample_kernel      one wave per virtual trajectory (row, slot, sample): lanes 0..3 run the Philox blocks of the state and the
//                         mass, every lane the 6 x 6 factor (wave-uniform), lane k the Gates draw of thrust node k -> y0, the thrust
//                         table and what the flight needs of the object.  The catalogue side of a catalogue call is a second launch.
//   propagate             FlightSet::fly on the virtual constellation, as mpcx_avoidance_window_refine flies
//   mc_scan_kernel        one wave per (row, sample), lane l scan interval l (l + 64, ...): both flown objects at the interval's ends
//                         by tr_state's Hermite, cj_interval's rule on the relative cubic (mc_interval), integer butterflies
//                         -> the sample's record (three int32 in the workspace; the optional `samples` row)
//   mc_accumulate_kernel  the chunk's records summed into counts [n][MPCX_NMCC]: per block a stride over the samples, the integer
//                         butterfly, four waves through LDS, one 64-bit atomicAdd per column -- integers, so any order gives the same
//   mc_copy_kernel        the optional Y_samples / U_samples
//   mc_finish_kernel      out [n][MPCX_NMC] and the final status from the counts.  One lane per row.
// Every draw is Philox4x32-10 on the counter (sample, object, block, side): it does not depend on the list, the row, the chunk or
// the launch.  All launches go onto one stream; their number is fixed by the arguments; nothing is read back.
// tests/collision_mc_reference.py restates the generator, the draws and the scan.
#include "collision_window_device.hpp"
#include "covariance_device.hpp"
#include "encounter_host.hpp"

#include <math.h>

namespace mpcx {

enum { MC_DEFAULT_FLIGHTS = 1 << 18 };                               // virtual trajectories in flight at once when max_flights = 0

// ---------------------------------------------------------------- the generator

// Philox4x32-10 (Salmon et al. 2011): counter c, key k -> four words
__device__ __forceinline__ void mc_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&o)[4])
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
        c0 = n0; c1 = l1; c2 = n2; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

// 53 bits of two words as a uniform: ((a >> 5) 2^26 + (b >> 6) + 0.5) 2^-53, strictly inside (0, 1).  Above 2^52 the + 0.5 is rounded
// to even; with all 53 bits set the exact value 1 - 2^-54 lies midway between 1 - 2^-53 and 1 and is rounded DOWN (the fmin).
__device__ __forceinline__ double mc_uniform(uint32_t a, uint32_t b)
{
    const double k = (double)(a >> 5) * 67108864.0 + (double)(b >> 6);
    const double kh = k + 0.5;
    return fmin(kh * 0x1p-53, 0x1.fffffffffffffp-1);
}

// the two normals of one Philox block (Box-Muller): words (0, 1) the radius, words (2, 3) the angle
__device__ __forceinline__ void mc_normals(uint32_t sample, uint32_t obj, uint32_t block, uint32_t side, uint32_t k0, uint32_t k1, double &za,
                                           double &zb)
{
    uint32_t w[4];
    mc_philox(sample, obj, block, side, k0, k1, w);
    const double u1 = mc_uniform(w[0], w[1]), u2 = mc_uniform(w[2], w[3]);
    const double lg = log(u1);
    const double rad = sqrt(-2.0 * lg);
    const double ang = 6.283185307179586 * u2;
    double sn, cs;
    sincos(ang, &sn, &cs);
    za = rad * cs; zb = rad * sn;
}

// ---------------------------------------------------------------- the factor

#define MC_L(i, j) L[(i) * ((i) + 1) / 2 + (j)]

// P0 = L L^T by columns (the upper triangle of P0 is read, L is the packed lower triangle), for a positive SEMI-definite P0.  With
// d_j = P0_jj - sum_k<j L_jk^2 and c_ij = P0_ji - sum_k<j L_ik L_jk (sums in ascending k) and tol_j = 1e-12 P0_jj:
//   d_j > tol_j            L_jj = sqrt(d_j), L_ij = c_ij / L_jj
//   |d_j| <= tol_j         a zero pivot: column j of L is zero, and every c_ij^2 <= tol_j P0_ii is required (a semi-definite matrix has
//                          them zero)
//   otherwise, or a diagonal entry that is negative or not finite: no factor (false).
__device__ __forceinline__ bool mc_factor(const double *P, double (&L)[21])
{
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const double tj = P[j * 6 + j];
        if (!(tj >= 0.0) || !cp_finite(tj)) ok = false;
        double d = tj;
#pragma unroll
        for (int k = 0; k < j; ++k) d = d - MC_L(j, k) * MC_L(j, k);
        const double tol = 1e-12 * tj;
        const bool reg = d > tol;
        if (!reg && !(d >= -tol)) ok = false;
        const double ljj = reg ? sqrt(d) : 0.0;
        MC_L(j, j) = ljj;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double c = P[j * 6 + i];
#pragma unroll
            for (int k = 0; k < j; ++k) c = c - MC_L(i, k) * MC_L(j, k);
            if (!reg && !(c * c <= tol * P[i * 6 + i])) ok = false;
            MC_L(i, j) = reg ? c / ljj : 0.0;
        }
    }
    return ok;
}

// ---------------------------------------------------------------- the problem

// one side of the list as the sampler takes it: the given plan and what is drawn about it
struct McSide {
    int N, K;
    const int32_t *Ks;
    const double *Y, *U, *units, *span, *consts, *P0, *exec, *mvar;
};

// The virtual constellation of one sampler launch is a FlightSet (encounter_host.hpp): V = n slots C trajectories,
// v = (r slots + slot) C + c, rows of length K.

// the flight's tf of an object and whether it is one
__device__ __forceinline__ bool mc_tf(const McSide &sd, int o, double &tf) { return tr_tf(sd.span[2 * o], sd.span[2 * o + 1], sd.units[2 * o + 1], tf); }

// what is drawn about object o can be drawn: the factor, a mass variance and an exec row that are finite and not negative
__device__ __forceinline__ bool mc_drawable(const McSide &sd, int o)
{
    double L[21];
    bool ok = mc_factor(sd.P0 + (size_t)o * 36, L);
    if (sd.mvar) { const double m = sd.mvar[o]; ok = ok && m >= 0.0 && cp_finite(m); }
    if (sd.exec) ok = ok && gates_valid(gates_load(sd.exec + (size_t)o * MPCX_NEXEC));
    return ok;
}

struct McRowsArgs {
    int n;
    const double *pairs, *half;
    CpSide row, col;                  // the given trajectories with the radii (cw_row)
    McSide rs, cs;                    // the same two sides for the sampler
    double *info;                     // [n][3]: t_a, t_b, R
    int32_t *rowst;
};

__global__ __launch_bounds__(256) void mc_rows_kernel(McRowsArgs a)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= a.n) return;
    const double *row = a.pairs + (size_t)r * 4;
    double ta = cp_nan(), tb = cp_nan(), R = cp_nan();
    CpNode na, nb;
    int st = cw_row(a.row, a.col, row[0], row[1], row[3], a.half[r], ta, tb, R, na, nb);
    if (st == MPCX_ST_OK && R > 0.0) {                               // (no sphere: nothing is asked of the draws)
        double tf;
        if (!mc_tf(a.rs, na.o, tf) || !mc_tf(a.cs, nb.o, tf)) st = MPCX_ST_BADK;
        else if (!mc_drawable(a.rs, na.o) || !mc_drawable(a.cs, nb.o)) st = MPCX_ST_NUMERIC;
    }
    a.info[(size_t)r * 3] = ta; a.info[(size_t)r * 3 + 1] = tb; a.info[(size_t)r * 3 + 2] = R;
    a.rowst[r] = st;
}

// ---------------------------------------------------------------- the sampler

struct McSampleArgs {
    McSide sd;
    uint32_t side, k0, k1, s0;        // 0 constellation, 1 catalogue; the key; the chunk's first sample
    int n, slots, col0, C;            // slots of this launch per row, the pairs column of its slot 0, samples in the chunk
    const double *pairs;
    FlightSet g;
};

__global__ __launch_bounds__(64) void mc_sample_kernel(McSampleArgs a)
{
    const int v = blockIdx.x, lane = threadIdx.x;
    const int rs = v / a.C, c = v - rs * a.C, r = rs / a.slots, sl = rs - r * a.slots;
    const McSide &sd = a.sd;
    const double fidx = a.pairs[(size_t)r * 4 + a.col0 + sl];
    const int o = fidx >= 0.0 && fidx < (double)sd.N ? (int)fidx : 0;        // (a row that fails its tests flies object 0, unread)
    const uint32_t smp = a.s0 + (uint32_t)c;
    const size_t K = (size_t)sd.K;
    const int nn = sd.Ks ? sd.Ks[o] : sd.K;
    const double Lu = sd.units[2 * o], Vu = Lu / sd.units[2 * o + 1];
    // ---- blocks 0..2 the six state normals, block 3 the mass normal: lane b runs block b
    double za = 0.0, zb = 0.0;
    if (lane < 4) mc_normals(smp, (uint32_t)o, (uint32_t)lane, a.side, a.k0, a.k1, za, zb);
    double z[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) z[i] = __shfl((i & 1) ? zb : za, i >> 1);
    const double zm = __shfl(za, 3);
    double L[21];
    const bool drawn = mc_factor(sd.P0 + (size_t)o * 36, L);         // (a matrix without a factor: mc_rows_kernel has failed the row,
                                                                     //  and the flight starts from the first node as given)
    double xv = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double x = MC_L(i, 0) * z[0];
#pragma unroll
        for (int j = 1; j <= i; ++j) x = x + MC_L(i, j) * z[j];
        if (lane == i) xv = x / (i < 3 ? Lu : Vu);
    }
    if (lane == 6) xv = sqrt(sd.mvar ? sd.mvar[o] : 0.0) * zm;
    if (!drawn || !cp_finite(xv)) xv = 0.0;                          // (a negative variance, a unit of zero: the row has failed as well)
    if (lane < 7) a.g.y0[(size_t)v * 7 + lane] = sd.Y[((size_t)o * 7 + lane) * K] + xv;
    if (lane < MPCX_NCONST) a.g.consts[(size_t)v * MPCX_NCONST + lane] = sd.consts[(size_t)o * MPCX_NCONST + lane];
    if (lane == 0) {
        double tf;
        a.g.Ks[v] = nn;
        a.g.tf[v] = mc_tf(sd, o, tf) ? tf : 1.0;
        a.g.end_tau[v] = 1.0;
    }
    // ---- the thrust table: lane k node k; blocks 4 + 2k and 5 + 2k its three normals
    GatesRow ex{};
    if (sd.exec) ex = gates_load(sd.exec + (size_t)o * MPCX_NEXEC);
    double *ut = a.g.Ut + (size_t)v * 3 * K;
    for (int k = lane; k < sd.K; k += 64) {
        double ux = 0.0, uy = 0.0, uz = 0.0;
        if (k < nn && sd.U) {
            const double *u = sd.U + (size_t)o * 3 * K;
            ux = u[k]; uy = u[K + k]; uz = u[2 * K + k];
            const double un = sqrt(ux * ux + uy * uy + uz * uz);
            if (sd.exec && gates_on(ex, un)) {
                double z1, z2, z3, zu;
                mc_normals(smp, (uint32_t)o, 4u + 2u * (uint32_t)k, a.side, a.k0, a.k1, z1, z2);
                mc_normals(smp, (uint32_t)o, 5u + 2u * (uint32_t)k, a.side, a.k0, a.k1, z3, zu);
                const double hx = ux / un, hy = uy / un, hz = uz / un;
                double vpar, vperp;
                gates_variances(ex, un, vpar, vperp);
                const double spar = sqrt(vpar), sperp = sqrt(vperp);
                // e_1: the coordinate axis on which |u^| is smallest (the first of equal ones), made orthogonal to u^ (cp_frame's rule)
                int ax = 0;
                double ea = hx;
                if (fabs(hy) < fabs(ea)) { ax = 1; ea = hy; }
                if (fabs(hz) < fabs(ea)) { ax = 2; ea = hz; }
                double e1x = (ax == 0 ? 1.0 : 0.0) - ea * hx, e1y = (ax == 1 ? 1.0 : 0.0) - ea * hy, e1z = (ax == 2 ? 1.0 : 0.0) - ea * hz;
                const double en = sqrt(e1x * e1x + e1y * e1y + e1z * e1z);
                e1x = e1x / en; e1y = e1y / en; e1z = e1z / en;
                const double e2x = hy * e1z - hz * e1y, e2y = hz * e1x - hx * e1z, e2z = hx * e1y - hy * e1x;
                const double a1 = spar * z1, a2 = sperp * z2, a3 = sperp * z3;
                ux = ux + (a1 * hx + (a2 * e1x + a3 * e2x));
                uy = uy + (a1 * hy + (a2 * e1y + a3 * e2y));
                uz = uz + (a1 * hz + (a2 * e1z + a3 * e2z));
            }
        }
        ut[k] = ux; ut[K + k] = uy; ut[2 * K + k] = uz;
    }
}

// ---------------------------------------------------------------- the scan

// position p (m) and velocity v (m/s) at time t of a flown trajectory y [7][ld] with nn nodes over [ta, tb]: tr_state, as cp_state
// without its tests -- the caller's t lies in the span
__device__ __forceinline__ void mc_state(const double *y, size_t ld, int nn, double ta, double tb, double L, double Tu, double t,
                                         double (&p)[3], double (&v)[3])
{
    const TrNode at = tr_locate(nn, ta, tb, t);
    double h00, h10, h01, h11;
    tr_value_basis(at.sg, h00, h10, h01, h11);
    tr_state(y, ld, at, h00, h10, h01, h11, L, L / Tu, p, v);
}

// One scan interval of length h from t0: the relative position is the cubic Hermite of the end differences d0, d1 and the end
// relative velocities w0, w1.  q0, q1: the squared distances at the ends; (qm, tm): the smallest squared distance found and its time
// by conjunction.hip's cj_interval rule -- the ends (the later one only if strictly smaller), then the interior point of tr_chord_start
// and tr_newton, only if strictly smaller.  (Its time is formed in two statements, t0 + (s h) rounded twice, where cj_interval's one
// expression is contracted: each keeps its own.)
__device__ __forceinline__ void mc_interval(const double (&d0)[3], const double (&d1)[3], const double (&w0)[3], const double (&w1)[3], double h,
                                            double t0, double t1, double &q0, double &q1, double &qm, double &tm)
{
    q0 = cp_dot(d0, d0); q1 = cp_dot(d1, d1);
    qm = q0; tm = t0;
    if (q1 < qm) { qm = q1; tm = t1; }
    double s = tr_chord_start(d0, d1);
    if (s > 0.0 && s < 1.0) {
        double a0[3], a1[3], x[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) { a0[c] = h * w0[c]; a1[c] = h * w1[c]; }
        for (int it = 0; it < 4; ++it) {                             // tr_newton's loop, kept as text: through the call mc_scan_kernel's
            double h00, h10, h01, h11;                               // register count moves (194 -> 192)
            tr_value_basis(s, h00, h10, h01, h11);
#pragma unroll
            for (int c = 0; c < 3; ++c) x[c] = h00 * d0[c] + h10 * a0[c] + h01 * d1[c] + h11 * a1[c];
            if (it == 3) break;
            double g00, g10, g01, g11;
            tr_slope_basis(s, g00, g10, g01, g11);
            const double k00 = 12.0 * s - 6.0, k10 = 6.0 * s - 4.0, k01 = -12.0 * s + 6.0, k11 = 6.0 * s - 2.0;
            double x1[3], x2[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                x1[c] = g00 * d0[c] + g10 * a0[c] + g01 * d1[c] + g11 * a1[c];
                x2[c] = k00 * d0[c] + k10 * a0[c] + k01 * d1[c] + k11 * a1[c];
            }
            const double g = cp_dot(x, x1), gp = cp_dot(x1, x1) + cp_dot(x, x2);
            if (gp > 0.0) {
                s = s - g / gp;
                s = s < 0.0 ? 0.0 : (s > 1.0 ? 1.0 : s);
            }
        }
        const double qs = cp_dot(x, x);
        const double ts = s * h;
        if (qs < qm) { qm = qs; tm = t0 + ts; }
    }
}

__device__ __forceinline__ int mc_wave_sum(int x)
{
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) x = x + __shfl_xor(x, sh);
    return x;
}

enum { MC_SKIP = -1 };                                               // a record's flight status where the row has no samples to count

struct McScanArgs {
    int n, C, N, scan, slots;         // slots of the row side per row (2: the column object is slot 1 of `a`; 1: it is in `b`)
    uint32_t s0;
    const double *pairs, *info;
    const int32_t *rowst;
    McSide rs, cs;
    FlightSet a, b;
    int32_t *rec;                     // [n][C][3]: flight status (or MC_SKIP), inside_start, entries
    double *samples;                  // [n][N][MPCX_NMS] or NULL
};

__global__ __launch_bounds__(64) void mc_scan_kernel(McScanArgs a)
{
    const int w = blockIdx.x, lane = threadIdx.x;
    const int r = w / a.C, c = w - r * a.C;
    const double ta = a.info[(size_t)r * 3], tb = a.info[(size_t)r * 3 + 1], R = a.info[(size_t)r * 3 + 2];
    const int rst = a.rowst[r];
    int32_t *rec = a.rec + (size_t)w * 3;
    double *smp = a.samples ? a.samples + ((size_t)r * a.N + a.s0 + c) * MPCX_NMS : nullptr;
    if (rst != MPCX_ST_OK || !(R > 0.0)) {                           // (wave-uniform) a failed row: NaN; no sphere: zeros
        if (lane == 0) {
            rec[0] = MC_SKIP; rec[1] = 0; rec[2] = 0;
            if (smp) {
                const double f = rst != MPCX_ST_OK ? cp_nan() : 0.0;
                smp[MPCX_MS_DMIN] = f; smp[MPCX_MS_T_MIN] = f; smp[MPCX_MS_INSIDE_START] = 0.0; smp[MPCX_MS_ENTRIES] = 0.0;
                smp[MPCX_MS_STATUS] = 0.0;
            }
        }
        return;
    }
    const double *row = a.pairs + (size_t)r * 4;
    const int oi = (int)row[0], oj = (int)row[1];                    // (tested by cw_row)
    const size_t vi = ((size_t)r * a.slots) * a.C + c, vj = a.slots == 2 ? ((size_t)r * 2 + 1) * a.C + c : (size_t)r * a.C + c;
    const FlightSet &gj = a.slots == 2 ? a.a : a.b;
    int fst = a.a.pst[vi];
    if (fst == MPCX_ST_OK) fst = gj.pst[vj];
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    double best = inf, tbest = ta;
    int ins = 0, ent = 0;
    if (fst == MPCX_ST_OK) {
        const size_t Ki = (size_t)a.rs.K, Kj = (size_t)a.cs.K;
        const double *yi = a.a.Yp + vi * 7 * Ki, *yj = gj.Yp + vj * 7 * Kj;
        const int ni = a.a.Ks[vi], nj = gj.Ks[vj];
        const double sai = a.rs.span[2 * oi], sbi = a.rs.span[2 * oi + 1], Li = a.rs.units[2 * oi], Ti = a.rs.units[2 * oi + 1];
        const double saj = a.cs.span[2 * oj], sbj = a.cs.span[2 * oj + 1], Lj = a.cs.units[2 * oj], Tj = a.cs.units[2 * oj + 1];
        const double R2 = R * R, hs = (tb - ta) / (double)a.scan;
        for (int m0 = 0; m0 < a.scan; m0 += 64) {
            const bool act = m0 + lane < a.scan;
            const int m = act ? m0 + lane : a.scan - 1;
            const double o0 = (double)m * hs, o1 = (double)(m + 1) * hs;
            const double t0 = ta + o0, t1 = m + 1 == a.scan ? tb : ta + o1;
            double pi[3], wi[3], pj[3], wj[3], d0[3], d1[3], w0[3], w1[3];
            mc_state(yi, Ki, ni, sai, sbi, Li, Ti, t0, pi, wi);
            mc_state(yj, Kj, nj, saj, sbj, Lj, Tj, t0, pj, wj);
#pragma unroll
            for (int x = 0; x < 3; ++x) { d0[x] = pj[x] - pi[x]; w0[x] = wj[x] - wi[x]; }
            mc_state(yi, Ki, ni, sai, sbi, Li, Ti, t1, pi, wi);
            mc_state(yj, Kj, nj, saj, sbj, Lj, Tj, t1, pj, wj);
#pragma unroll
            for (int x = 0; x < 3; ++x) { d1[x] = pj[x] - pi[x]; w1[x] = wj[x] - wi[x]; }
            double q0, q1, qm, tm;
            mc_interval(d0, d1, w0, w1, t1 - t0, t0, t1, q0, q1, qm, tm);
            ent = ent + mc_wave_sum(act && q0 > R2 && (q1 <= R2 || qm <= R2) ? 1 : 0);
            if (m0 == 0) ins = __shfl(q0 <= R2 ? 1 : 0, 0);
            const double qa = act && qm == qm ? qm : inf;
            const double pm = -cp_wave_max(-qa);
            const double te = -cp_wave_max(qa == pm ? -tm : -inf);  // the earliest of equal ones
            if (pm < best) { best = pm; tbest = te; }
        }
        if (!(best < inf)) fst = MPCX_ST_NUMERIC;                    // a flight that came back without a number
    }
    if (lane == 0) {
        const bool ok = fst == MPCX_ST_OK;
        rec[0] = fst; rec[1] = ok ? ins : 0; rec[2] = ok ? ent : 0;
        if (smp) {
            smp[MPCX_MS_DMIN] = ok ? sqrt(best) : cp_nan(); smp[MPCX_MS_T_MIN] = ok ? tbest : cp_nan();
            smp[MPCX_MS_INSIDE_START] = ok ? (double)ins : 0.0; smp[MPCX_MS_ENTRIES] = ok ? (double)ent : 0.0;
            smp[MPCX_MS_STATUS] = (double)fst;
        }
    }
}

// ---------------------------------------------------------------- the counts

__device__ __forceinline__ long long mc_wave_sum64(long long x)
{
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) x = x + __shfl_xor(x, sh);
    return x;
}

// grid (n, blocks per row) -- the rows on x, whose limit a long list does not reach: block b of row r takes the chunk's samples
// b 256 + t, stride gridDim.y 256
__global__ __launch_bounds__(256) void mc_accumulate_kernel(int C, const int32_t *rec, long long *counts)
{
    __shared__ long long part[4][MPCX_NMCC];
    const int r = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    long long s[MPCX_NMCC];
#pragma unroll
    for (int e = 0; e < MPCX_NMCC; ++e) s[e] = 0;
    for (int c = blockIdx.y * 256 + t; c < C; c += gridDim.y * 256) {
        const int32_t *q = rec + ((size_t)r * C + c) * 3;
        const int fst = q[0];
        if (fst == MC_SKIP) continue;
        const long long in = q[1], en = q[2], bd = in + en;
        s[MPCX_MCC_FLOWN] += 1;
        s[MPCX_MCC_FAILED] += fst != MPCX_ST_OK ? 1 : 0;
        s[MPCX_MCC_START] += in; s[MPCX_MCC_ENTRIES] += en; s[MPCX_MCC_SQUARES] += bd * bd; s[MPCX_MCC_HIT] += bd >= 1 ? 1 : 0;
    }
#pragma unroll
    for (int e = 0; e < MPCX_NMCC; ++e) {
        const long long x = mc_wave_sum64(s[e]);
        if (lane == 0) part[wv][e] = x;
    }
    __syncthreads();
    if (t < MPCX_NMCC) {
        const long long x = (part[0][t] + part[1][t]) + (part[2][t] + part[3][t]);
        if (x != 0) atomicAdd((unsigned long long *)(counts + (size_t)r * MPCX_NMCC + t), (unsigned long long)x);
    }
}

__global__ __launch_bounds__(256) void mc_finish_kernel(int n, const double *info, const int32_t *rowst, long long *counts, double *out,
                                                        int32_t *status)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const double ta = info[(size_t)r * 3], tb = info[(size_t)r * 3 + 1], R = info[(size_t)r * 3 + 2];
    long long *cn = counts + (size_t)r * MPCX_NMCC;
    double *o = out + (size_t)r * MPCX_NMC;
    int st = rowst[r];
    const long long nok = cn[MPCX_MCC_FLOWN] - cn[MPCX_MCC_FAILED];
    const bool empty = st == MPCX_ST_OK && !(R > 0.0);
    if (st == MPCX_ST_OK && !empty && nok < 1) st = MPCX_ST_NUMERIC;       // no sample survived its flight
    if (st != MPCX_ST_OK) {                                          // a failed row: NaN, and zero in counts
        for (int e = 0; e < MPCX_NMC; ++e) o[e] = cp_nan();
        for (int e = 0; e < MPCX_NMCC; ++e) cn[e] = 0;
    } else if (empty) {
        for (int e = 0; e < MPCX_NMC; ++e) o[e] = 0.0;
        o[MPCX_MC_TA] = ta; o[MPCX_MC_TB] = tb;
    } else {
        const double N = (double)nok;
        const double p = (double)cn[MPCX_MCC_HIT] / N, start = (double)cn[MPCX_MCC_START] / N, entries = (double)cn[MPCX_MCC_ENTRIES] / N;
        const double sb = (double)(cn[MPCX_MCC_START] + cn[MPCX_MCC_ENTRIES]), sq = (double)cn[MPCX_MCC_SQUARES];
        const double dev = sq - sb * sb / N;                         // sum (b - mean b)^2
        const double var = nok > 1 && dev > 0.0 ? dev / (N - 1.0) : 0.0;
        o[MPCX_MC_P_HIT] = p; o[MPCX_MC_SE_HIT] = sqrt(p * (1.0 - p) / N);
        o[MPCX_MC_START] = start; o[MPCX_MC_ENTRIES] = entries; o[MPCX_MC_SE_BOUND] = sqrt(var / N);
        o[MPCX_MC_EXCESS] = (start + entries) - p;
        o[MPCX_MC_TA] = ta; o[MPCX_MC_TB] = tb; o[MPCX_MC_N_OK] = N;
    }
    status[r] = st;
}

// ---------------------------------------------------------------- the optional trajectories

// src [V][per = rows K] of a chunk -> dst [n slots][N][rows][K] at the chunk's samples.  A failed row and (pst given) a failed flight
// are NaN; columns past the trajectory's node count are zero.
__global__ __launch_bounds__(256) void mc_copy_kernel(size_t total, int rows, int K, int slots, int C, int N, uint32_t s0, const double *src,
                                                      const int32_t *Ks, const int32_t *pst, const int32_t *rowst, double *dst)
{
    const size_t per = (size_t)rows * K;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t v = e / per, x = e - v * per, rs = v / C, c = v - rs * C;
        const bool bad = rowst[rs / slots] != MPCX_ST_OK || (pst && pst[v] != MPCX_ST_OK);
        const int k = (int)(x % K);
        dst[(rs * N + s0 + c) * per + x] = bad ? cp_nan() : (k >= Ks[v] ? 0.0 : src[e]);
    }
}

// ---------------------------------------------------------------- the host side

// the geometry (no P, cat_P or mu: the covariances are sampled from P0) plus the truth model, the sampling and the outputs
struct McCall : EncGeometry {
    const double *U, *consts;
    int flags;
    double prop_max_step;
    const double *P0, *exec, *m_var0, *cat_consts, *cat_P0;
    const double *half;
    int scan, n_samples;
    uint64_t seed;
    int max_flights;
    int64_t *counts;
    double *out;
    int32_t *status;
    double *samples, *Y_samples, *U_samples;
};

static const char *const MC_NAME = "collision_probability_mc";

// samples per chunk: floor(max_flights / (n NS)), at least one, at most all
static int mc_chunk(int n, int NS, int n_samples, int max_flights)
{
    const long long mf = max_flights > 0 ? max_flights : MC_DEFAULT_FLIGHTS;
    long long cs = mf / ((long long)n * NS);
    if (cs < 1) cs = 1;
    return (int)(cs < n_samples ? cs : n_samples);
}

static int mc_check(mpcx_ctx *ctx, const McCall &c)
{
    if (c.n < 1 || c.S < 1 || c.K < 2) return enc_fail(ctx, MC_NAME, "need n>=1, S>=1, K>=2");
    if (!(c.prop_max_step > 0.0)) return enc_fail(ctx, MC_NAME, "prop_max_step must be > 0");
    if (c.flags & ~(MPCX_FLAG_DRAG | MPCX_FLAG_J2 | MPCX_FLAG_ATMO))
        return enc_fail(ctx, MC_NAME, "flags are MPCX_FLAG_DRAG | MPCX_FLAG_J2 | MPCX_FLAG_ATMO");
    if (c.scan < 1) return enc_fail(ctx, MC_NAME, "scan must be >= 1");
    if (c.n_samples < 1) return enc_fail(ctx, MC_NAME, "n_samples must be >= 1");
    if (c.max_flights < 0) return enc_fail(ctx, MC_NAME, "max_flights is 0 (the default) or > 0");
    if (!c.pairs || !c.Y || !c.units || !c.span || !c.consts || !c.P0 || !c.radius || !c.half || !c.counts || !c.out || !c.status)
        return enc_fail(ctx, MC_NAME, "pairs, Y, units, span, consts, P0, radius, half_window, counts, out and status are required");
    if (int rc = geom_check_catalogue(ctx, c, MC_NAME, c.cat_consts && c.cat_P0 && c.cat_radius,
                                      "cat_units, cat_span, cat_consts, cat_P0 and cat_radius"))
        return rc;
    const int NS = c.cat_Y ? 1 : 2;
    if ((long long)c.n * 2 * mc_chunk(c.n, NS, c.n_samples, c.max_flights) > 0x7fffffffLL)
        return enc_fail(ctx, MC_NAME, "too many virtual trajectories in one chunk: lower max_flights or split the list");
    return ctx_check_atmosphere(ctx, c.flags, MC_NAME);
}

// [the rows' window, R and status][the chunk's records][the row side's virtual constellation][the catalogue side's]
struct McWorkspace {
    double *info;
    int32_t *rowst, *rec;
    FlightSet a, b;
    size_t bytes;
    McWorkspace(void *base, int n, int K, bool cat, int cat_K, int Cs)
    {
        Carver c(base);
        info = c.take<double>((size_t)n * 3);
        rowst = c.take<int32_t>((size_t)n);
        rec = c.take<int32_t>((size_t)n * Cs * 3);
        a.carve(c, (size_t)n * (cat ? 1 : 2) * Cs, (size_t)K);
        b = FlightSet{};
        if (cat) b.carve(c, (size_t)n * Cs, (size_t)cat_K);
        bytes = c.bytes();
    }
};

// device pointers throughout in `c`
static int mc_enqueue(mpcx_ctx *ctx, const McCall &c, void *workspace, hipStream_t st)
{
    const bool cat = c.cat_Y != nullptr;
    const int n = c.n, K = c.K, NS = cat ? 1 : 2, N = c.n_samples, Cs = mc_chunk(n, NS, N, c.max_flights);
    const McWorkspace ws(workspace, n, K, cat, c.cat_K, Cs);
    const McSide rs{c.S, K, c.Ks, c.Y, c.U, c.units, c.span, c.consts, c.P0, c.exec, c.m_var0};
    const McSide cs = cat ? McSide{c.D, c.cat_K, c.cat_Ks, c.cat_Y, nullptr, c.cat_units, c.cat_span, c.cat_consts, c.cat_P0, nullptr, nullptr} : rs;
    CpSide row, col;
    enc_sides(c, row, col);
    const uint32_t k0 = (uint32_t)(c.seed & 0xffffffffu), k1 = (uint32_t)(c.seed >> 32);
    const unsigned gn = (unsigned)((n + 255) / 256);
    long long *counts = (long long *)c.counts;
    MPCX_HIP(ctx, hipMemsetAsync(counts, 0, (size_t)n * MPCX_NMCC * sizeof(long long), st));
    hipLaunchKernelGGL(mc_rows_kernel, dim3(gn), dim3(256), 0, st, McRowsArgs{n, c.pairs, c.half, row, col, rs, cs, ws.info, ws.rowst});
    MPCX_HIP(ctx, hipGetLastError());
    for (int s0 = 0; s0 < N; s0 += Cs) {
        const int C = N - s0 < Cs ? N - s0 : Cs, Va = n * NS * C, Vb = n * C;
        hipLaunchKernelGGL(mc_sample_kernel, dim3((unsigned)Va), dim3(64), 0, st,
                           McSampleArgs{rs, 0u, k0, k1, (uint32_t)s0, n, NS, 0, C, c.pairs, ws.a});
        MPCX_HIP(ctx, hipGetLastError());
        if (int rc = ws.a.fly(ctx, Va, K, c.flags, c.prop_max_step, st)) return rc;
        if (cat) {
            hipLaunchKernelGGL(mc_sample_kernel, dim3((unsigned)Vb), dim3(64), 0, st,
                               McSampleArgs{cs, 1u, k0, k1, (uint32_t)s0, n, 1, 1, C, c.pairs, ws.b});
            MPCX_HIP(ctx, hipGetLastError());
            if (int rc = ws.b.fly(ctx, Vb, c.cat_K, c.flags, c.prop_max_step, st)) return rc;
        }
        hipLaunchKernelGGL(mc_scan_kernel, dim3((unsigned)(n * C)), dim3(64), 0, st,
                           McScanArgs{n, C, N, c.scan, NS, (uint32_t)s0, c.pairs, ws.info, ws.rowst, rs, cs, ws.a, ws.b, ws.rec, c.samples});
        MPCX_HIP(ctx, hipGetLastError());
        const unsigned gb = (unsigned)((C + 4095) / 4096 < 64 ? (C + 4095) / 4096 : 64);
        hipLaunchKernelGGL(mc_accumulate_kernel, dim3((unsigned)n, gb), dim3(256), 0, st, C, ws.rec, counts);
        MPCX_HIP(ctx, hipGetLastError());
        for (int which = 0; which < 2; ++which) {
            double *dst = which ? c.U_samples : c.Y_samples;
            if (!dst) continue;
            const int rows = which ? 3 : 7;
            const size_t total = (size_t)Va * rows * K;
            const size_t blocks = (total + 255) / 256;
            hipLaunchKernelGGL(mc_copy_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, st, total, rows, K, NS, C, N,
                               (uint32_t)s0, which ? ws.a.Ut : ws.a.Yp, ws.a.Ks, which ? nullptr : ws.a.pst, ws.rowst, dst);
            MPCX_HIP(ctx, hipGetLastError());
        }
    }
    hipLaunchKernelGGL(mc_finish_kernel, dim3(gn), dim3(256), 0, st, n, ws.info, ws.rowst, counts, c.out, c.status);
    MPCX_HIP(ctx, hipGetLastError());
    return MPCX_OK;
}

}  // namespace mpcx

using namespace mpcx;

extern "C" size_t mpcx_collision_probability_mc_workspace_bytes(int n, int S, int K, int D, int cat_K, int n_samples, int max_flights)
{
    if (n < 1 || S < 1 || K < 2 || D < 0 || (D > 0 && cat_K < 2) || n_samples < 1 || max_flights < 0) return 0;
    return McWorkspace(nullptr, n, K, D > 0, cat_K, mc_chunk(n, D > 0 ? 1 : 2, n_samples, max_flights)).bytes;
}

// the arguments of the two entry points below as a McCall
#define MPCX_MC_CALL                                                                                                                        \
    McCall{{n, pairs, S, K, Ks, Y, units, span, nullptr, radius, D, cat_K, cat_Ks, cat_Y, cat_units, cat_span, nullptr, cat_radius, 0.0}, \
           U, consts, flags, prop_max_step, P0, exec, m_var0, cat_consts, cat_P0, half_window, scan, n_samples, seed, max_flights, counts,  \
           out, status, samples, Y_samples, U_samples}

extern "C" int mpcx_collision_probability_mc_dev(mpcx_ctx *ctx, int n, const double *pairs, int S, int K, const int32_t *Ks, const double *Y,
                                                 const double *U, const double *units, const double *span, const double *consts, int flags,
                                                 double prop_max_step, const double *P0, const double *exec, const double *m_var0,
                                                 const double *radius, int D, int cat_K, const int32_t *cat_Ks, const double *cat_Y,
                                                 const double *cat_units, const double *cat_span, const double *cat_consts,
                                                 const double *cat_P0, const double *cat_radius, const double *half_window, int scan,
                                                 int n_samples, uint64_t seed, int max_flights, int64_t *counts, double *out,
                                                 int32_t *status, double *samples, double *Y_samples, double *U_samples, void *workspace,
                                                 void *stream)
{
    if (!ctx) return MPCX_E_BADARG;
    const McCall c = MPCX_MC_CALL;
    if (int rc = mc_check(ctx, c)) return rc;
    if (!workspace)
        return enc_fail(ctx, MC_NAME,
                        "a workspace of mpcx_collision_probability_mc_workspace_bytes(n, S, K, D, cat_K, n_samples, max_flights) bytes is required");
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    return mc_enqueue(ctx, c, workspace, (hipStream_t)stream);
}

extern "C" int mpcx_collision_probability_mc(mpcx_ctx *ctx, int n, const double *pairs, int S, int K, const int32_t *Ks, const double *Y,
                                             const double *U, const double *units, const double *span, const double *consts, int flags,
                                             double prop_max_step, const double *P0, const double *exec, const double *m_var0,
                                             const double *radius, int D, int cat_K, const int32_t *cat_Ks, const double *cat_Y,
                                             const double *cat_units, const double *cat_span, const double *cat_consts, const double *cat_P0,
                                             const double *cat_radius, const double *half_window, int scan, int n_samples, uint64_t seed,
                                             int max_flights, int64_t *counts, double *out, int32_t *status, double *samples,
                                             double *Y_samples, double *U_samples)
{
    if (!ctx) return MPCX_E_BADARG;
    const McCall c = MPCX_MC_CALL;
    if (int rc = mc_check(ctx, c)) return rc;
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    DeviceArena ar(ctx);
    McCall d = c;
    const size_t Sz = (size_t)S, Kz = (size_t)K, Dz = (size_t)D, nz = (size_t)n, N = (size_t)n_samples, NS = cat_Y ? 1 : 2;
    geom_upload(ar, d);
    d.half = ar.upload(half_window, nz); d.U = U ? ar.upload(U, Sz * 3 * Kz) : nullptr; d.consts = ar.upload(consts, Sz * MPCX_NCONST);
    d.P0 = ar.upload(P0, Sz * 36); d.exec = exec ? ar.upload(exec, Sz * MPCX_NEXEC) : nullptr;
    d.m_var0 = m_var0 ? ar.upload(m_var0, Sz) : nullptr;
    if (cat_Y) { d.cat_consts = ar.upload(cat_consts, Dz * MPCX_NCONST); d.cat_P0 = ar.upload(cat_P0, Dz * 36); }
    d.counts = ar.result(counts, nz * MPCX_NMCC);
    d.out = ar.result(out, nz * MPCX_NMC);
    d.status = ar.result(status, nz);
    d.samples = ar.result(samples, nz * N * MPCX_NMS);
    d.Y_samples = ar.result(Y_samples, nz * NS * N * 7 * Kz);
    d.U_samples = ar.result(U_samples, nz * NS * N * 3 * Kz);
    return host_run(ctx, ar, mpcx_collision_probability_mc_workspace_bytes(n, S, K, cat_Y ? D : 0, cat_K, n_samples, max_flights),
                    [&](void *ws, hipStream_t st) { return mc_enqueue(ctx, d, ws, st); });
}
#undef MPCX_MC_CALL
