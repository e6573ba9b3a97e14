// avoidance_joint.hip -- all of a satellite's encounters under its thrust limit (include/mpcx.h: mpcx_avoidance_joint*).
//   aj_rows_kernel    one wave per listed pair: the encounter frame, the adjoint sweep over A | B_kn | B_kp and the g_m of the ONE object
//                     that moves -- the functions of collision_device.hpp that avoidance_kernel (avoidance.hip) calls too, so that with
//                     W = I the row has the bits of mpcx_avoidance's sens -- contracted to the tangent half-plane row a_p and its
//                     right-hand side.
//   aj_solve_kernel   one wave per satellite that has rows: its row indices in ascending list order, the terminal sweep (the same
//                     recursion with six rows, seeded [I_6 | 0] at the last node), and the strictly convex problem by the semismooth
//                     Newton iteration of the header: a lane-strided pass over the nodes for du(z) and the projection's Jacobian, one
//                     lane per entry of H and of the residual (sums over the nodes in ascending order), a Cholesky in LDS.
// Nothing crosses a workgroup; every sum runs in ascending index order or in the xor butterfly's fixed order: the results depend on
// the inputs alone (tests/avoidance_joint_reference.py restates them).  Plain vector loads and stores throughout.
// At the end of the file: mpcx_avoidance_refine*, the loop around the joint call (fly, re-screen, linearise, solve again), which gives
// aj_solve_kernel a reference thrust, a terminal right-hand side and a warm start -- all absent in the joint call itself.
#include "collision_device.hpp"
#include "encounter_host.hpp"

#include <string.h>
#include <vector>

namespace mpcx {

enum { AJ_MAXR = MPCX_AJ_MAX_ROWS, AJ_NZ = 6 + MPCX_AJ_MAX_ROWS, AJ_LINE_SEARCH = 30 };
enum { AJI_D0 = 0, AJI_B, AJI_Q1, AJI_Q2, AJI_MN, AJI_WN, AJI_W11, AJI_W12, AJI_W22, AJ_INFO = 10 };      // per-pair record of the workspace
#define AJ_PIVOT_REL 1e-12

struct AjArgs {
    int n, S, K, sat0, nsat, have_cat, have_P, hold, max_iter;
    const double *pairs;
    const int32_t *mover;             // [n] or NULL
    CpSide row, col;
    const double *U;                  // [S][3][K]
    const double *stage;              // [S][K-1][MPCX_STAGE_DOUBLES]
    const int32_t *dstat;             // the discretiser's status [S]
    const double *u_max;              // [S] or NULL
    double mu, target, tol;
    double *g;                        // workspace [n][3][3][K]: the g_m of the object that moves
    double *a;                        // [n][3][K]: `rows` when the caller gave it, otherwise the workspace
    double *info;                     // workspace [n][AJ_INFO]
    int32_t *owner;                   // workspace [n]: the satellite a row belongs to, -1: none
    double *T;                        // [S][6][3][K]: `tsens` when the caller gave it, otherwise the workspace
    int zero_T;                       // T is tsens: what the sweep does not reach is part of the result
    double *jd;                       // workspace [S][6][K]: the projection's Jacobian over D_m, upper triangle
    double *du, *sat_out, *row_out;
    int32_t *sat_status, *row_status;
    // the refinement's inputs of aj_solve_kernel (mpcx_avoidance_refine); all absent in the joint call, whose code they leave alone
    const double *uref = nullptr;     // [S][3][K]: the centre of the ball projection and the origin of the effort (NULL: U)
    const double *trhs = nullptr;     // [S][6]: the terminal rows' right-hand side (NULL: 0)
    const double *z0 = nullptr;       // [S][AJ_NZ]: the start of the iteration, y then lambda * target in row order (NULL: 0)
    double *z_out = nullptr;          // [S][AJ_NZ]: the converged z (may be z0)
    const int32_t *skip = nullptr;    // [S]: not 0: the satellite is left alone, nothing of it is written
    int T_ready = 0;                  // T holds the terminal sweep already (ar_trhs_kernel ran it)
    double *rhs_rows = nullptr;       // [n]: the encounter rows' right-hand sides as solved, in the rows' own units
    double *rhs_term = nullptr;       // [S][6]: the terminal rows'
};

__global__ __launch_bounds__(64) void aj_rows_kernel(AjArgs a)
{
    __shared__ double rec[CP_REC_PAD], lam[24];
    const int pr = blockIdx.x, lane = threadIdx.x;
    if (pr >= a.n) return;
    const double *row = a.pairs + (size_t)pr * 4;
    const double t = row[3];
    const size_t K = (size_t)a.K;
    const int mvr = a.mover ? a.mover[pr] : 0;
    const double fm = mvr ? row[1] : row[0];
    const bool mover_ok = (mvr == 0 || (mvr == 1 && !a.have_cat)) && fm >= 0.0 && fm < (double)a.S;
    const int own = mover_ok ? (int)fm : -1;
    if (lane == 0) a.owner[pr] = own;
    // a call computes the rows of its own block of satellites; a row nobody owns is reported by the block that starts at satellite 0
    if (own < 0 ? a.sat0 != 0 : (own < a.sat0 || own >= a.sat0 + a.nsat)) return;
    double *g = a.g + (size_t)pr * 9 * K, *ar = a.a + (size_t)pr * 3 * K;

    // ---- both objects at t, the statuses that end the row, the encounter frame and the target's metric (wave-uniform)
    double pa[3], va[3], pb[3], vb[3];
    CpNode nda, ndb;
    int st = mover_ok ? MPCX_ST_OK : MPCX_ST_BADK;
    if (st == MPCX_ST_OK) st = cp_state(a.row, row[0], t, pa, va, nda);
    if (st == MPCX_ST_OK) st = cp_state(a.col, row[1], t, pb, vb, ndb);
    CpMover mv = {};
    const CpNode &ndm = mvr ? ndb : nda;                             // (the object that moves is one of the constellation: the row side)
    if (st == MPCX_ST_OK) st = cp_mover(a.row, a.dstat, ndm, K, mv);
    double ew[3], e1[3], e2[3], mn = 0.0, wn = 0.0, W11 = 1.0, W12 = 0.0, W22 = 1.0;
    if (st == MPCX_ST_OK) {
        double d[3], w[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) { d[c] = pb[c] - pa[c]; w[c] = vb[c] - va[c]; }
        st = cp_frame(d, w, wn, ew, mn, e1, e2);
        if (st == MPCX_ST_OK && a.have_P) {
            double Ca[6], Cb[6], Cs[6];
            CpPlane pl;
            cp_covariance(a.row, nda, t, a.mu, Ca);
            cp_covariance(a.col, ndb, t, a.mu, Cb);
#pragma unroll
            for (int c = 0; c < 6; ++c) Cs[c] = Ca[c] + Cb[c];
            st = cp_plane_covariance(Cs, e1, e2, pl);
            if (st == MPCX_ST_OK) { W11 = pl.c22 / pl.det; W12 = -pl.c12 / pl.det; W22 = pl.c11 / pl.det; }      // W = C_2^-1
        }
    }

    double o[MPCX_NAR];
#pragma unroll
    for (int c = 0; c < MPCX_NAR; ++c) o[c] = cp_nan();
    if (st == MPCX_ST_OK) {
        // ---- the adjoint sweep of the object that moves, seeded with R Lam of the two bracketing nodes, entry (lr, lc)
        const int lr = lane < 21 ? lane / 7 : 0, lc = lane < 21 ? lane - 7 * (lane / 7) : 0;
        double seed_hi = 0.0, seed_lo = 0.0;
        cp_sweep_seed(mvr ? 1.0 : -1.0, e1, e2, ew, mv.L, mv.htau, ndm.h00, ndm.h10, ndm.h01, ndm.h11, lr, lc, seed_hi, seed_lo);
        for (int e = 0; e < 9; ++e)                                  // the nodes past k + 1
            for (int m = mv.k + 2 + lane; m < a.K; m += 64) g[(size_t)e * K + m] = 0.0;
        aj_sweep<3>(lane, a.stage + (size_t)mv.o * (K - 1) * MPCX_STAGE_DOUBLES, mv.k, seed_hi, seed_lo, g, K, rec, lam);

        // ---- the tangent half-plane of the target ellipse: q = W (1, 0)^T / sqrt(W11), a_m = q_1 g_m[0, :] + q_2 g_m[1, :]
        const double sq = sqrt(W11), q1 = W11 / sq, q2 = W12 / sq;
        const double d0 = sqrt(mn * W11 * mn);
        for (int c = 0; c < 3; ++c)
            for (int m = lane; m < a.K; m += 64) {
                const double g0 = g[(size_t)c * K + m];
                ar[(size_t)c * K + m] = a.have_P ? q1 * g0 + q2 * g[(size_t)(3 + c) * K + m] : g0;
            }
        if (lane == 0) {
            double *in = a.info + (size_t)pr * AJ_INFO;
            in[AJI_D0] = d0; in[AJI_B] = a.target - d0; in[AJI_Q1] = q1; in[AJI_Q2] = q2; in[AJI_MN] = mn; in[AJI_WN] = wn;
            in[AJI_W11] = W11; in[AJI_W12] = W12; in[AJI_W22] = W22;
        }
        o[MPCX_AR_D0] = d0;
    } else {
        for (size_t e = lane; e < 3 * K; e += 64) ar[e] = cp_nan();
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < MPCX_NAR; ++c) a.row_out[(size_t)pr * MPCX_NAR + c] = o[c];
        a.row_status[pr] = st;
    }
}

// what the passes over the nodes need of the satellite (wave-uniform)
struct AjSat {
    int ns, ne, r, nz;
    double hn, cfac, umax, target;
    bool ball;
    const double *mass, *ctr, *T;     // Y[s][6][.], the centre of the projection (U[s]; uref[s] when given), T[s]
    const double *trhs;               // the terminal rows' right-hand side [6] or NULL
    double *du, *jd;
    const double *a;                  // all rows [n][3][K]
    size_t K;
};

// entry (component c, node m) of constraint row i: the terminal rows first, then the encounter rows.  The problem takes an encounter
// row in units of the target; the division is applied once to the row's multiplier, residual and entries of H, not to every entry.
__device__ __forceinline__ double aj_entry(const AjSat &sa, const int *idx, int i, int c, int m)
{
    return i < sa.ne ? sa.T[((size_t)i * 3 + c) * sa.K + m] : sa.a[((size_t)idx[i - sa.ne] * 3 + c) * sa.K + m];
}

// du(z) at every node and the projection's Jacobian over D_m, then F(z) = [T du; min(c lambda, slack)]: slack (LDS, r), F (LDS, nz).
// Returns max |F|, NaN when an entry is not finite.  nball: this lane's count of nodes on the ball.
__device__ __forceinline__ double aj_evaluate(const AjSat &sa, const int *idx, const double *z, const double *bh, const double *cs, double *F,
                                              double *slack, int lane, int &nball)
{
    nball = 0;
    for (int m = lane; m < sa.ns; m += 64) {
        double v[3] = {0.0, 0.0, 0.0};
        for (int i = 0; i < sa.nz; ++i) {
            const double zi = i < sa.ne ? z[i] : z[i] / sa.target;
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = v[c] + zi * aj_entry(sa, idx, i, c, m);
        }
        const double cm = sa.cfac / sa.mass[m];
        const double wm = (m == 0 || m == sa.ns - 1) ? 0.5 * sa.hn : sa.hn;
        const double D = wm * cm * cm;
        double ub[3], p[3], J[6] = {1.0, 0.0, 0.0, 1.0, 0.0, 1.0};                       // (00, 01, 02, 11, 12, 22)
#pragma unroll
        for (int c = 0; c < 3; ++c) { ub[c] = sa.ctr[(size_t)c * sa.K + m]; p[c] = ub[c] + v[c] / D; }
        const double pn = sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
        if (sa.ball && pn > sa.umax) {
            const double sc = sa.umax / pn;
            const double ph[3] = {p[0] / pn, p[1] / pn, p[2] / pn};
            J[0] = sc * (1.0 - ph[0] * ph[0]); J[1] = sc * (0.0 - ph[0] * ph[1]); J[2] = sc * (0.0 - ph[0] * ph[2]);
            J[3] = sc * (1.0 - ph[1] * ph[1]); J[4] = sc * (0.0 - ph[1] * ph[2]); J[5] = sc * (1.0 - ph[2] * ph[2]);
#pragma unroll
            for (int c = 0; c < 3; ++c) p[c] = p[c] * sc;
            ++nball;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) sa.du[(size_t)c * sa.K + m] = p[c] - ub[c];
#pragma unroll
        for (int e = 0; e < 6; ++e) sa.jd[(size_t)e * sa.K + m] = J[e] / D;
    }
    __syncthreads();
    if (lane < sa.nz) {
        double res = 0.0;
        for (int m = 0; m < sa.ns; ++m)
            res = res + (aj_entry(sa, idx, lane, 0, m) * sa.du[m] + aj_entry(sa, idx, lane, 1, m) * sa.du[sa.K + m]
                         + aj_entry(sa, idx, lane, 2, m) * sa.du[2 * sa.K + m]);
        if (lane < sa.ne) F[lane] = sa.trhs ? res - sa.trhs[lane] : res;
        else {
            const double s = res / sa.target - bh[lane - sa.ne];
            slack[lane - sa.ne] = s;
            F[lane] = fmin(cs[lane - sa.ne] * z[lane], s);
            if (!cp_finite(z[lane]) || !cp_finite(s)) F[lane] = cp_nan();
        }
    }
    __syncthreads();
    double mF = 0.0;
    bool bad = false;
    for (int i = 0; i < sa.nz; ++i) {
        const double f = fabs(F[i]);
        if (!cp_finite(f)) bad = true;
        mF = fmax(mF, f);
    }
    return bad ? cp_nan() : mF;
}

__global__ __launch_bounds__(64) void aj_solve_kernel(AjArgs a)
{
    __shared__ double rec[CP_REC_PAD], lam[48];
    __shared__ double z[AJ_NZ], zn[AJ_NZ], dz[AJ_NZ], F[AJ_NZ], slack[AJ_MAXR], bh[AJ_MAXR], cs[AJ_MAXR], gd[AJ_NZ];
    __shared__ double H[AJ_NZ][AJ_NZ], G[AJ_NZ][AJ_NZ + 1];
    __shared__ int idx[AJ_MAXR], act[AJ_NZ];
    const int lane = threadIdx.x;
    if ((int)blockIdx.x >= a.nsat) return;
    const int s = a.sat0 + (int)blockIdx.x;
    if (a.skip && a.skip[s]) return;
    const size_t K = (size_t)a.K;
    double *du = a.du + (size_t)s * 3 * K, *so = a.sat_out + (size_t)s * MPCX_NAJ;
    double *Ts = a.T + (size_t)s * 18 * K;

    // ---- the satellite's rows in ascending list order, and the first status among them that is not OK
    int cnt = 0, st = MPCX_ST_OK;
    for (int base = 0; base < a.n; base += 64) {
        const int p = base + lane;
        const bool mine = p < a.n && a.owner[p] == s;
        unsigned long long mask = __ballot(mine);
        while (mask) {
            const int bit = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            const int q = base + bit;
            if (cnt < AJ_MAXR && lane == 0) idx[cnt] = q;
            if (st == MPCX_ST_OK) st = a.row_status[q];
            ++cnt;
        }
    }
    __syncthreads();
    if (st == MPCX_ST_OK && cnt > AJ_MAXR) st = MPCX_ST_BADK;
    const int r = cnt > AJ_MAXR ? AJ_MAXR : cnt;

    if (cnt == 0 || st != MPCX_ST_OK) {                              // nothing to do, or nothing that can be done
        const double fill = cnt == 0 ? 0.0 : cp_nan();
        for (size_t e = lane; e < 3 * K; e += 64) du[e] = fill;
        if (a.zero_T)
            for (size_t e = lane; e < 18 * K; e += 64) Ts[e] = 0.0;
        if (lane < MPCX_NAJ) so[lane] = fill;
        if (lane == 0) a.sat_status[s] = st;
        return;
    }

    // (a row that is OK has checked the satellite's node count, span, tf and linearisation)
    AjSat sa;
    sa.ns = a.row.Ks ? a.row.Ks[s] : a.K;
    sa.ne = a.hold ? 6 : 0; sa.r = r; sa.nz = sa.ne + r;
    const double L = a.row.units[2 * s], Tu = a.row.units[2 * s + 1];
    sa.hn = (a.row.span[2 * s + 1] - a.row.span[2 * s]) / (double)(sa.ns - 1);
    sa.cfac = L / (Tu * Tu);
    sa.umax = a.u_max ? a.u_max[s] : __longlong_as_double(0x7ff0000000000000LL);
    sa.ball = sa.umax < __longlong_as_double(0x7ff0000000000000LL);
    sa.target = a.target;
    sa.mass = a.row.Y + ((size_t)s * 7 + 6) * K; sa.ctr = (a.uref ? a.uref : a.U) + (size_t)s * 3 * K; sa.T = Ts;
    sa.trhs = a.trhs ? a.trhs + (size_t)s * 6 : nullptr;
    sa.du = du; sa.jd = a.jd + (size_t)s * 6 * K; sa.a = a.a; sa.K = K;
    const int nz = sa.nz, ne = sa.ne, ns = sa.ns;

    for (int c = 0; c < 3; ++c)                                      // nodes past ns
        for (int m = ns + lane; m < a.K; m += 64) du[(size_t)c * K + m] = 0.0;
    if (a.hold && a.T_ready) {
        // (the terminal sweep is in T already)
    } else if (a.hold) {
        // ---- the terminal sweep: lam_ns-1 = [I_6 | 0], over the whole horizon
        for (int e = 0; e < 18; ++e)
            for (int m = ns + lane; m < a.K; m += 64) Ts[(size_t)e * K + m] = 0.0;
        const int lr = lane < 42 ? lane / 7 : 0, lc = lane < 42 ? lane - 7 * (lane / 7) : 0;
        aj_sweep<6>(lane, a.stage + (size_t)s * (K - 1) * MPCX_STAGE_DOUBLES, ns - 2, lane < 42 && lr == lc ? 1.0 : 0.0, 0.0, Ts, K, rec, lam);
    } else if (a.zero_T) {
        for (size_t e = lane; e < 18 * K; e += 64) Ts[e] = 0.0;
    }

    // ---- a row the ball alone forbids: sum_m (u_max |a_m| - a_m . ubar_m) < b
    //      (with a reference thrust the unknown is the change from uref while the row is linearised about U: b + sum_m a_m . (U_m - uref_m))
    double brow = 0.0;
    if (lane < r) {
        brow = a.info[(size_t)idx[lane] * AJ_INFO + AJI_B];
        if (a.uref) {
            const double *ap = a.a + (size_t)idx[lane] * 3 * K, *ul = a.U + (size_t)s * 3 * K;
            double sh = 0.0;
            for (int m = 0; m < ns; ++m)
                sh = sh + (ap[m] * (ul[m] - sa.ctr[m]) + ap[K + m] * (ul[K + m] - sa.ctr[K + m]) + ap[2 * K + m] * (ul[2 * K + m] - sa.ctr[2 * K + m]));
            brow = brow + sh;
        }
        bh[lane] = brow / a.target;
        if (a.rhs_rows) a.rhs_rows[idx[lane]] = brow;
    }
    if (a.rhs_term && lane < 6) a.rhs_term[(size_t)s * 6 + lane] = sa.trhs && a.hold ? sa.trhs[lane] : 0.0;
    bool infeasible = false;
    if (sa.ball && lane < r) {
        const double *ap = a.a + (size_t)idx[lane] * 3 * K;
        double reach = 0.0;
        for (int m = 0; m < ns; ++m) {
            const double a0 = ap[m], a1 = ap[K + m], a2 = ap[2 * K + m];
            reach = reach + (sa.umax * sqrt(a0 * a0 + a1 * a1 + a2 * a2) - (a0 * sa.ctr[m] + a1 * sa.ctr[K + m] + a2 * sa.ctr[2 * K + m]));
        }
        infeasible = reach < brow;
    }
    if (__ballot(infeasible)) st = MPCX_ST_INFEASIBLE;
    // ---- a row's own authority c_p = sum_m |a_p,m / target|^2 / D_m: what a multiplier of 1 moves the row by when it acts alone
    if (lane < r) {
        const double *ap = a.a + (size_t)idx[lane] * 3 * K;
        double c = 0.0;
        for (int m = 0; m < ns; ++m) {
            const double cm = sa.cfac / sa.mass[m];
            const double wm = (m == 0 || m == ns - 1) ? 0.5 * sa.hn : sa.hn;
            const double a0 = ap[m] / a.target, a1 = ap[K + m] / a.target, a2 = ap[2 * K + m] / a.target;
            c = c + (a0 * a0 + a1 * a1 + a2 * a2) / (wm * cm * cm);
        }
        cs[lane] = c;
    }

    // ---- the semismooth Newton iteration on F(z) = [T du(z); min(c lambda, (a du(z) - b) / target)]
    int iters = 0, nball = 0;
    double mF = 0.0;
    if (st == MPCX_ST_OK) {
        if (lane < nz) z[lane] = a.z0 ? a.z0[(size_t)s * AJ_NZ + (lane < ne ? lane : 6 + lane - ne)] : 0.0;
        __syncthreads();
        mF = aj_evaluate(sa, idx, z, bh, cs, F, slack, lane, nball);
        for (;;) {
            if (!cp_finite(mF)) { st = MPCX_ST_MAXITER; break; }
            // the active rows, and whether this is the solution: F small, an inactive row's multiplier exactly 0, none negative
            if (lane < nz) act[lane] = lane < ne || cs[lane - ne] * z[lane] > slack[lane - ne];
            __syncthreads();
            bool done = mF <= a.tol;
            for (int i = ne; i < nz; ++i)
                if ((!act[i] && z[i] != 0.0) || z[i] < 0.0) done = false;
            if (done) break;
            if (iters == a.max_iter) { st = MPCX_ST_MAXITER; break; }
            // H = sum_m A_m J_m A_m^T / D_m, one lane per entry of the upper triangle, the nodes in ascending order
            for (int e = lane; e < nz * (nz + 1) / 2; e += 64) {
                int i = 0, rem = e;
                while (rem >= nz - i) { rem -= nz - i; ++i; }
                const int j = i + rem;
                double h = 0.0;
                for (int m = 0; m < ns; ++m) {
                    const double x0 = aj_entry(sa, idx, i, 0, m), x1 = aj_entry(sa, idx, i, 1, m), x2 = aj_entry(sa, idx, i, 2, m);
                    const double y0 = aj_entry(sa, idx, j, 0, m), y1 = aj_entry(sa, idx, j, 1, m), y2 = aj_entry(sa, idx, j, 2, m);
                    const double *jm = sa.jd + m;
                    const double J00 = jm[0], J01 = jm[K], J02 = jm[2 * K], J11 = jm[3 * K], J12 = jm[4 * K], J22 = jm[5 * K];
                    h = h + (x0 * (J00 * y0 + J01 * y1 + J02 * y2) + x1 * (J01 * y0 + J11 * y1 + J12 * y2) + x2 * (J02 * y0 + J12 * y1 + J22 * y2));
                }
                if (i >= ne) h = h / a.target;
                if (j >= ne) h = h / a.target;
                H[i][j] = h; H[j][i] = h;
            }
            __syncthreads();
            // G dz = rhs: the Newton step on the active rows, dz = -lambda on the inactive ones
            double rv = 0.0;
            if (lane < nz) {
                if (act[lane]) {
                    rv = -F[lane];
                    for (int j = ne; j < nz; ++j)
                        if (!act[j]) rv = rv + H[lane][j] * z[j];
                } else rv = -z[lane];
                for (int j = 0; j < nz; ++j) G[lane][j] = act[lane] && act[j] ? H[lane][j] : (lane == j ? 1.0 : 0.0);
                gd[lane] = act[lane] ? H[lane][lane] : 1.0;
            }
            __syncthreads();
            bool singular = false;
            for (int j = 0; j < nz && !singular; ++j) {              // Cholesky, right-looking, row i on lane i
                const double d = G[j][j];
                if (!(d > AJ_PIVOT_REL * gd[j])) { singular = true; break; }
                const double sd = sqrt(d);
                double lij = 0.0;
                if (lane > j && lane < nz) lij = G[lane][j] / sd;
                __syncthreads();
                if (lane > j && lane < nz) G[lane][j] = lij;
                if (lane == j) G[j][j] = sd;
                __syncthreads();
                if (lane > j && lane < nz)
                    for (int k = j + 1; k <= lane; ++k) G[lane][k] = G[lane][k] - lij * G[k][j];
                __syncthreads();
            }
            if (singular) { st = MPCX_ST_SINGULAR; break; }
            for (int j = 0; j < nz; ++j) {                           // L y = rhs
                const double yj = __shfl(rv, j) / G[j][j];
                if (lane == j) rv = yj;
                else if (lane > j && lane < nz) rv = rv - G[lane][j] * yj;
            }
            for (int j = nz - 1; j >= 0; --j) {                      // L^T dz = y
                const double xj = __shfl(rv, j) / G[j][j];
                if (lane == j) rv = xj;
                else if (lane < j) rv = rv - G[j][lane] * xj;
            }
            if (lane < nz) dz[lane] = rv;
            __syncthreads();
            // halve the step on max |F| (t = 1 takes an inactive row's multiplier to 0 exactly)
            double tstep = 1.0, mFn = 0.0;
            bool ok = false;
            for (int ls = 0; ls < AJ_LINE_SEARCH; ++ls) {
                if (lane < nz) zn[lane] = z[lane] + tstep * dz[lane];
                __syncthreads();
                mFn = aj_evaluate(sa, idx, zn, bh, cs, F, slack, lane, nball);
                if (mFn < mF || mFn <= a.tol) { ok = true; break; }
                tstep = 0.5 * tstep;
            }
            ++iters;
            if (!ok) { st = MPCX_ST_MAXITER; break; }
            if (lane < nz) z[lane] = zn[lane];
            mF = mFn;
            __syncthreads();
        }
    }

    if (st != MPCX_ST_OK) {                                          // defined results: NaN
        for (size_t e = lane; e < 3 * K; e += 64) du[e] = cp_nan();
        if (lane < MPCX_NAJ) so[lane] = cp_nan();
        if (lane == 0) a.sat_status[s] = st;
        return;
    }

    // ---- what the manoeuvre costs and where it ends
    double scost = 0.0, sdv = 0.0, smax = 0.0;
    for (int m = lane; m < ns; m += 64) {
        const double cm = sa.cfac / sa.mass[m];
        const double wm = (m == 0 || m == ns - 1) ? 0.5 * sa.hn : sa.hn;
        const double d0 = du[m], d1 = du[K + m], d2 = du[2 * K + m];
        const double u0 = sa.ctr[m] + d0, u1 = sa.ctr[K + m] + d1, u2 = sa.ctr[2 * K + m] + d2;
        const double da0 = cm * d0, da1 = cm * d1, da2 = cm * d2;
        scost = scost + (wm * cm * cm) * (d0 * d0 + d1 * d1 + d2 * d2);
        sdv = sdv + wm * sqrt(da0 * da0 + da1 * da1 + da2 * da2);
        smax = fmax(smax, sqrt(u0 * u0 + u1 * u1 + u2 * u2));
    }
    const double cost = 0.5 * cp_wave_sum(scost), dv = cp_wave_sum(sdv), umx = cp_wave_max(smax), nb = cp_wave_sum((double)nball);
    int nact = 0;
    for (int i = ne; i < nz; ++i) nact += z[i] > 0.0 ? 1 : 0;
    if (lane == 0) {
        so[MPCX_AJ_COST] = cost; so[MPCX_AJ_DV] = dv; so[MPCX_AJ_UMAX] = umx; so[MPCX_AJ_ROWS] = (double)r; so[MPCX_AJ_ACTIVE] = (double)nact;
        so[MPCX_AJ_ONBALL] = nb; so[MPCX_AJ_ITERS] = (double)iters; so[MPCX_AJ_RESIDUAL] = mF;
        a.sat_status[s] = st;
    }
    if (a.z_out && lane < nz) a.z_out[(size_t)s * AJ_NZ + (lane < ne ? lane : 6 + lane - ne)] = z[lane];
    // ---- per row: the displacement in the frame, g_m du_m summed over the nodes (lane 4 p + c: rows e_1, e_2, e_w of g, then a)
    double sum = 0.0;
    if (lane < 4 * r) {
        const int p = lane >> 2, c = lane & 3;
        const double *gp = c < 3 ? a.g + ((size_t)idx[p] * 9 + (size_t)c * 3) * K : a.a + (size_t)idx[p] * 3 * K;
        if (a.uref) {                                                // from the linearisation's thrust: uref + du - U
            const double *ul = a.U + (size_t)s * 3 * K;
            for (int m = 0; m < ns; ++m)
                sum = sum + (gp[m] * (du[m] - (ul[m] - sa.ctr[m])) + gp[K + m] * (du[K + m] - (ul[K + m] - sa.ctr[K + m]))
                             + gp[2 * K + m] * (du[2 * K + m] - (ul[2 * K + m] - sa.ctr[2 * K + m])));
        } else
            for (int m = 0; m < ns; ++m) sum = sum + (gp[m] * du[m] + gp[K + m] * du[K + m] + gp[2 * K + m] * du[2 * K + m]);
    }
    const int p4 = (lane >> 2) << 2;
    const double dm1 = __shfl(sum, p4), dm2 = __shfl(sum, p4 + 1), along = __shfl(sum, p4 + 2), adu = __shfl(sum, p4 + 3);
    if (lane < 4 * r && (lane & 3) == 0) {
        const int p = lane >> 2;
        const double *in = a.info + (size_t)idx[p] * AJ_INFO;
        double *ro = a.row_out + (size_t)idx[p] * MPCX_NAR;
        const double x1 = in[AJI_MN] + dm1, W11 = in[AJI_W11], W12 = in[AJI_W12], W22 = in[AJI_W22];
        ro[MPCX_AR_MARGIN] = in[AJI_D0] + adu;
        ro[MPCX_AR_DIST] = sqrt(x1 * (W11 * x1 + W12 * dm2) + dm2 * (W12 * x1 + W22 * dm2));
        ro[MPCX_AR_LAMBDA] = z[ne + p] / a.target;
        ro[MPCX_AR_DT] = -along / in[AJI_WN];
    }
}

// The refinement's terminal right-hand side (mpcx_avoidance_refine): the terminal sweep of the pass's linearisation into T -- the solve
// that follows finds it there (T_ready) -- and trhs = sum_m T_m du_prev_m - (Y_t[0:6, ns-1] - Y0[0:6, ns-1]), the nodes in ascending
// order: the end state is held to the GIVEN plan's.  One wave per satellite that is still refined (its node count was checked by the
// rows of the first pass).
__global__ __launch_bounds__(64) void ar_trhs_kernel(AjArgs a, const double *du_prev, const double *Y0, double *trhs)
{
    __shared__ double rec[CP_REC_PAD], lam[48];
    const int lane = threadIdx.x, s = blockIdx.x;
    if (s >= a.S || (a.skip && a.skip[s])) return;
    const size_t K = (size_t)a.K;
    const int ns = a.row.Ks ? a.row.Ks[s] : a.K;
    if (ns < 2 || ns > a.K) return;
    double *Ts = a.T + (size_t)s * 18 * K;
    for (int e = 0; e < 18; ++e)
        for (int m = ns + lane; m < a.K; m += 64) Ts[(size_t)e * K + m] = 0.0;
    const int lr = lane < 42 ? lane / 7 : 0, lc = lane < 42 ? lane - 7 * (lane / 7) : 0;
    aj_sweep<6>(lane, a.stage + (size_t)s * (K - 1) * MPCX_STAGE_DOUBLES, ns - 2, lane < 42 && lr == lc ? 1.0 : 0.0, 0.0, Ts, K, rec, lam);
    if (lane < 6) {
        const double *tp = Ts + (size_t)lane * 3 * K, *dp = du_prev + (size_t)s * 3 * K;
        double t = 0.0;
        for (int m = 0; m < ns; ++m) t = t + (tp[m] * dp[m] + tp[K + m] * dp[K + m] + tp[2 * K + m] * dp[2 * K + m]);
        const size_t e = ((size_t)s * 7 + lane) * K + (ns - 1);
        trhs[(size_t)s * 6 + lane] = t - (a.row.Y[e] - Y0[e]);
    }
}

// workspace of the _dev call: [the linearisation's][g n 3 3 K][a n 3 K][info n][owner n][T S 6 3 K][jd S 6 K]
struct AjWorkspace : LinWorkspace {
    double *g, *a, *info, *T, *jd;
    int32_t *owner;
    size_t bytes;
    AjWorkspace(void *base, int n, int S, int K)
    {
        Carver c(base);
        carve(c, S, K);
        g = c.take<double>((size_t)n * 9 * K);
        a = c.take<double>((size_t)n * 3 * K);
        info = c.take<double>((size_t)n * AJ_INFO);
        owner = c.take<int32_t>((size_t)n);
        T = c.take<double>((size_t)S * 18 * K);
        jd = c.take<double>((size_t)S * 6 * K);
        bytes = c.bytes();
    }
};

struct AjCall : EncProblem {
    const int32_t *mover;
    const double *u_max;
    int hold_terminal;
    double tol;
    int max_iter, sat0, nsat;
    double *du, *sat_out, *row_out, *rows, *tsens;
    int32_t *sat_status, *row_status;
};

// the arguments of an entry point as an AjCall; SAT0, NSAT: the block of satellites it computes
#define MPCX_AJ_CALL(SAT0, NSAT)                                                                                                   \
    AjCall{MPCX_ENC_PROBLEM(nullptr, nullptr, target), mover, u_max, hold_terminal, tol, max_iter, SAT0, NSAT, du, sat_out, row_out, \
           rows, tsens, sat_status, row_status}

static int aj_check(mpcx_ctx *ctx, const AjCall &c)
{
    if (int rc = enc_check(ctx, c, "avoidance_joint", c.du && c.sat_out && c.row_out && c.sat_status && c.row_status,
                           "du, sat_out, row_out, sat_status and row_status"))
        return rc;
    if (!(c.tol > 0.0) || !(c.tol < __builtin_inf()) || c.max_iter < 1)
        return enc_fail(ctx, "avoidance_joint", "tol must be a positive finite number and max_iter >= 1");
    if (c.sat0 < 0 || c.nsat < 1 || c.sat0 > c.S - c.nsat)
        return enc_fail(ctx, "avoidance_joint", "the block sat0 .. sat0 + nsat - 1 must lie in 0 .. S - 1, nsat >= 1");
    return MPCX_OK;
}

// the device array of a result of the joint call: on its way back whole, or (a block of satellites) for the caller to download in parts
template <typename T> static T *aj_out(DeviceArena &ar, bool whole, T *host, size_t len)
{
    return whole ? ar.result(host, len) : host ? ar.alloc<T>(len) : nullptr;
}

// the problem's and the joint call's own host arrays replaced by copies on the device, and the device arrays of its results: they
// have the caller's shapes, whatever block of satellites the call computes
static void aj_stage(DeviceArena &ar, AjCall &d, bool whole)
{
    const size_t n = (size_t)d.n, S = (size_t)d.S, K = (size_t)d.K;
    enc_upload(ar, d);
    d.mover = d.mover ? ar.upload(d.mover, n) : nullptr;
    d.u_max = d.u_max ? ar.upload(d.u_max, S) : nullptr;
    d.du = aj_out(ar, whole, d.du, S * 3 * K);
    d.sat_out = aj_out(ar, whole, d.sat_out, S * MPCX_NAJ);
    d.row_out = aj_out(ar, whole, d.row_out, n * MPCX_NAR);
    d.rows = aj_out(ar, whole, d.rows, n * 3 * K);
    d.tsens = aj_out(ar, whole, d.tsens, S * 18 * K);
    d.sat_status = aj_out(ar, whole, d.sat_status, S);
    d.row_status = aj_out(ar, whole, d.row_status, n);
}

// what a pass of the refinement adds to the joint call (all NULL / 0 with solve = 1: the joint call)
struct AjPass {
    const double *uref = nullptr, *z0 = nullptr;
    double *z_out = nullptr;
    const int32_t *skip = nullptr;
    double *trhs = nullptr;           // [S][6] buffer: filled by ar_trhs_kernel from du_prev and Y0, then the solve's right-hand side
    const double *du_prev = nullptr, *Y0 = nullptr;
    double *rhs_rows = nullptr, *rhs_term = nullptr;
    int solve = 1;                    // 0: the rows alone (d0 of the last flight)
};

static int aj_enqueue(mpcx_ctx *ctx, const AjCall &c, void *workspace, hipStream_t st, const AjPass &x = AjPass())
{
    const AjWorkspace ws(workspace, c.n, c.S, c.K);
    if (int rc = enc_linearise(ctx, c, ws, st)) return rc;
    AjArgs a;
    a.n = c.n; a.S = c.S; a.K = c.K; a.sat0 = c.sat0; a.nsat = c.nsat; a.have_cat = c.cat_Y != nullptr; a.have_P = c.P != nullptr;
    a.hold = c.hold_terminal != 0; a.max_iter = c.max_iter;
    a.pairs = c.pairs; a.mover = c.mover;
    enc_sides(c, a.row, a.col);
    a.U = c.U; a.stage = ws.stage; a.dstat = ws.dstat; a.u_max = c.u_max;
    a.mu = c.mu; a.target = c.target; a.tol = c.tol;
    a.g = ws.g; a.a = c.rows ? c.rows : ws.a; a.info = ws.info; a.owner = ws.owner;
    a.T = c.tsens ? c.tsens : ws.T; a.zero_T = c.tsens != nullptr; a.jd = ws.jd;
    a.du = c.du; a.sat_out = c.sat_out; a.row_out = c.row_out; a.sat_status = c.sat_status; a.row_status = c.row_status;
    hipLaunchKernelGGL(aj_rows_kernel, dim3((unsigned)c.n), dim3(64), 0, st, a);
    MPCX_HIP(ctx, hipGetLastError());
    if (!x.solve) return MPCX_OK;
    a.uref = x.uref; a.z0 = x.z0; a.z_out = x.z_out; a.skip = x.skip; a.rhs_rows = x.rhs_rows; a.rhs_term = x.rhs_term;
    if (x.trhs && a.hold) {
        hipLaunchKernelGGL(ar_trhs_kernel, dim3((unsigned)c.S), dim3(64), 0, st, a, x.du_prev, x.Y0, x.trhs);
        MPCX_HIP(ctx, hipGetLastError());
        a.trhs = x.trhs; a.T_ready = 1;
    }
    hipLaunchKernelGGL(aj_solve_kernel, dim3((unsigned)c.nsat), dim3(64), 0, st, a);
    MPCX_HIP(ctx, hipGetLastError());
    return MPCX_OK;
}

}  // namespace mpcx

using namespace mpcx;

extern "C" size_t mpcx_avoidance_joint_workspace_bytes(int n, int S, int K)
{
    if (n < 1 || S < 1 || K < 2) return 0;
    return AjWorkspace(nullptr, n, S, K).bytes;
}

extern "C" int mpcx_avoidance_joint_dev(mpcx_ctx *ctx, int n, const double *pairs, const int32_t *mover, int S, int K, const int32_t *Ks,
                                        const double *Y, const double *U, const double *units, const double *span, const double *consts,
                                        int flags, double max_step, const double *P, int D, int cat_K, const int32_t *cat_Ks,
                                        const double *cat_Y, const double *cat_units, const double *cat_span, const double *cat_P, double mu,
                                        double target, const double *u_max, int hold_terminal, double tol, int max_iter, int sat0, int nsat,
                                        double *du, double *sat_out, double *row_out, double *rows, double *tsens, int32_t *sat_status,
                                        int32_t *row_status, void *workspace, void *stream)
{
    if (!ctx) return MPCX_E_BADARG;
    const AjCall c = MPCX_AJ_CALL(sat0, nsat);
    if (int rc = aj_check(ctx, c)) return rc;
    if (!workspace)
        return ctx_fail(ctx, MPCX_E_BADARG, "avoidance_joint: a workspace of mpcx_avoidance_joint_workspace_bytes(n, S, K) bytes is required");
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    return aj_enqueue(ctx, c, workspace, (hipStream_t)stream);
}

extern "C" int mpcx_avoidance_joint(mpcx_ctx *ctx, int n, const double *pairs, const int32_t *mover, int S, int K, const int32_t *Ks,
                                    const double *Y, const double *U, const double *units, const double *span, const double *consts, int flags,
                                    double max_step, const double *P, int D, int cat_K, const int32_t *cat_Ks, const double *cat_Y,
                                    const double *cat_units, const double *cat_span, const double *cat_P, double mu, double target,
                                    const double *u_max, int hold_terminal, double tol, int max_iter, int sat0, int nsat, double *du,
                                    double *sat_out, double *row_out, double *rows, double *tsens, int32_t *sat_status, int32_t *row_status)
{
    if (!ctx) return MPCX_E_BADARG;
    const AjCall c = MPCX_AJ_CALL(sat0, nsat);
    if (int rc = aj_check(ctx, c)) return rc;
    if (int rc = check_mover(ctx, c, mover, "avoidance_joint")) return rc;
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    DeviceArena ar(ctx);
    AjCall d = c;
    aj_stage(ar, d, false);
    if (ar.failed()) return ar.code();
    void *ws = ctx_workspace(ctx, mpcx_avoidance_joint_workspace_bytes(n, S, K));
    if (!ws) return MPCX_E_NOMEM;
    if (int rc = aj_enqueue(ctx, d, ws, ctx->stream)) return rc;
    const size_t s0 = (size_t)sat0, ns = (size_t)nsat;
    ar.download(du + s0 * 3 * K, d.du + s0 * 3 * K, ns * 3 * K);
    ar.download(sat_out + s0 * MPCX_NAJ, d.sat_out + s0 * MPCX_NAJ, ns * MPCX_NAJ);
    if (tsens) ar.download(tsens + s0 * 18 * K, d.tsens + s0 * 18 * K, ns * 18 * K);
    ar.download(sat_status + s0, d.sat_status + s0, ns);
    // the rows of the list: only those the block owns reach the caller's arrays (a row nobody owns: with the block that starts at 0)
    const bool whole = sat0 == 0 && nsat == S;
    std::vector<double> h_out, h_rows;
    std::vector<int32_t> h_st;
    if (!whole) {
        h_out.resize((size_t)n * MPCX_NAR); h_st.resize((size_t)n);
        if (rows) h_rows.resize((size_t)n * 3 * K);
    }
    ar.download(whole ? row_out : h_out.data(), d.row_out, (size_t)n * MPCX_NAR);
    ar.download(whole ? row_status : h_st.data(), d.row_status, (size_t)n);
    if (rows) ar.download(whole ? rows : h_rows.data(), d.rows, (size_t)n * 3 * K);
    if (int rc = ar.finish()) return rc;
    if (!whole)
        for (int r = 0; r < n; ++r) {
            const double fm = (mover && mover[r]) ? pairs[(size_t)r * 4 + 1] : pairs[(size_t)r * 4];
            const bool owned = fm >= 0.0 && fm < (double)S;
            if (owned ? ((int)fm < sat0 || (int)fm >= sat0 + nsat) : sat0 != 0) continue;
            memcpy(row_out + (size_t)r * MPCX_NAR, h_out.data() + (size_t)r * MPCX_NAR, MPCX_NAR * sizeof(double));
            row_status[r] = h_st[(size_t)r];
            if (rows) memcpy(rows + (size_t)r * 3 * K, h_rows.data() + (size_t)r * 3 * K, (size_t)3 * K * sizeof(double));
        }
    return MPCX_OK;
}

// ---- iterated avoidance: the manoeuvre flown, looked at and corrected again (include/mpcx.h: mpcx_avoidance_refine*)
//   pass 0            the joint call as it is
//   pass t >= 1       ar_apply_kernel   U_t = U + du_t-1 for a satellite that flies (rows and a finite du at pass 0), U otherwise
//                     propagate         every satellite from its first node under U_t
//                     ar_select_kernel  Y_t: the flight of a satellite that flies, the given trajectory otherwise; the end-state history;
//                                       a failed flight freezes the satellite
//                     the re-screen     mpcx_conjunction_pairs_traj_dev on Y_t: its out IS the pass's list.  Tracked (mpcx_avoidance_
//                                       refine_tracked*): mpcx_conjunction_track_traj_dev of the GIVEN list, whose column 3 is the time
//                                       each row follows in every pass -- a pair listed twice keeps its two encounters apart
//                     linearisation about (Y_t, U_t), aj_rows_kernel, ar_trhs_kernel, aj_solve_kernel (uref = U, z0 from the last solve)
//                                       into trial arrays; ar_accept_kernel takes them over or freezes the satellite
//   pass rounds + 1   the same without the solve: every answer is returned as flown
// Everything is enqueued on one stream; the number of passes is fixed, nothing is read back in between.  One block per satellite or
// one thread per element, no sum crosses a thread: the results depend on the inputs alone.
namespace mpcx {

__global__ __launch_bounds__(64) void ar_init_kernel(int S, int K, int n, const double *Y, const double *sat_out, const int32_t *sat_status,
                                                     int32_t *flies, int32_t *skip, int32_t *rounds_done, double *y0, double *end_tau,
                                                     double *hist_term, double *z, double *rhs_rows, double *rhs_term, int pass0)
{
    // pass0 = 1 (before the first solve): what the solve may leave unwritten; 0 (after it): who flies
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (pass0) {
        if (e < S * AJ_NZ) z[e] = 0.0;
        if (rhs_rows && e < n) rhs_rows[e] = cp_nan();
        if (rhs_term && e < S * 6) rhs_term[e] = 0.0;
        return;
    }
    if (e >= S) return;
    const int f = sat_status[e] == MPCX_ST_OK && sat_out[(size_t)e * MPCX_NAJ + MPCX_AJ_ROWS] > 0.0;
    flies[e] = f; skip[e] = !f; rounds_done[e] = f ? 0 : -1;
    for (int c = 0; c < 7; ++c) y0[(size_t)e * 7 + c] = Y[((size_t)e * 7 + c) * K];
    end_tau[e] = 1.0;
    hist_term[e] = 0.0;
}

__global__ __launch_bounds__(256) void ar_hist_kernel(int n, const double *row_out, const double *pairs, double *hist_d0, double *hist_tca)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    hist_d0[p] = row_out[(size_t)p * MPCX_NAR + MPCX_AR_D0];
    hist_tca[p] = pairs[(size_t)p * 4 + 3];
}

__global__ __launch_bounds__(256) void ar_apply_kernel(int S, int K, const double *U, const double *du, const int32_t *flies, double *Ut)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)S * 3 * K) return;
    const int s = (int)(e / ((size_t)3 * K));
    Ut[e] = flies[s] ? U[e] + du[e] : U[e];
}

__global__ __launch_bounds__(64) void ar_select_kernel(int S, int K, const int32_t *Ks, const double *Y, const double *Yp, const int32_t *pst,
                                                       const int32_t *flies, int32_t *skip, int32_t *sat_status, double *Yt, double *hist_term)
{
    const int s = blockIdx.x, lane = threadIdx.x;
    if (s >= S) return;
    const int ns = Ks ? Ks[s] : K;
    const bool flown = flies[s] && pst[s] == MPCX_ST_OK;
    const size_t base = (size_t)s * 7 * K;
    for (int e = lane; e < 7 * K; e += 64) {
        const int m = e % K;
        Yt[base + e] = flown ? (m < ns ? Yp[base + e] : 0.0) : Y[base + e];
    }
    if (lane == 0) {
        double dev = 0.0;
        if (flown)
            for (int c = 0; c < 6; ++c) dev = fmax(dev, fabs(Yp[base + (size_t)c * K + (ns - 1)] - Y[base + (size_t)c * K + (ns - 1)]));
        hist_term[s] = dev;
        if (flies[s] && !flown && !skip[s]) { skip[s] = 1; sat_status[s] = pst[s]; }       // a failed flight: frozen, du stays
    }
}

__global__ __launch_bounds__(64) void ar_accept_kernel(int n, int K, int t, const int32_t *owner, const double *du_try, const double *sat_try,
                                                       const double *row_try, const int32_t *sat_st_try, const int32_t *row_st_try,
                                                       int32_t *skip, double *du, double *sat_out, double *row_out, int32_t *sat_status,
                                                       int32_t *row_status, int32_t *rounds_done)
{
    const int s = blockIdx.x, lane = threadIdx.x;
    if (skip[s]) return;                                             // (wave-uniform; written below by lane 0 after everybody has read it)
    const int st = sat_st_try[s];
    __syncthreads();
    if (st != MPCX_ST_OK) {                                          // a failed solve: frozen, du stays, the status is reported
        if (lane == 0) { skip[s] = 1; sat_status[s] = st; }
        return;
    }
    for (int e = lane; e < 3 * K; e += 64) du[(size_t)s * 3 * K + e] = du_try[(size_t)s * 3 * K + e];
    if (lane < MPCX_NAJ) sat_out[(size_t)s * MPCX_NAJ + lane] = sat_try[(size_t)s * MPCX_NAJ + lane];
    for (int p = lane; p < n; p += 64)
        if (owner[p] == s) {
            for (int c = 0; c < MPCX_NAR; ++c) row_out[(size_t)p * MPCX_NAR + c] = row_try[(size_t)p * MPCX_NAR + c];
            row_status[p] = row_st_try[p];
        }
    if (lane == 0) { sat_status[s] = MPCX_ST_OK; rounds_done[s] = t; }
}

struct ArCall {
    AjCall j;
    int M;
    double T0, T1, prop_max_step;
    int rounds;
    double *Y_out, *pairs_out, *hist_d0, *hist_tca, *hist_term;
    int32_t *rounds_done;
    double *rhs_rows, *rhs_term;
    bool track = false;                                              // the re-screen follows each row's own encounter (track_kernel)
    double max_shift = 0.0;                                          //   at most this far from the row's given time; <= 0: unlimited
};

// [the joint call's workspace][the re-screen's][U_t S 3 K][flight S 7 K][y0 S 7][end_tau S][du S 3 K][sat_out S][row_out n][z S 14][trhs S 6]
// [flight status, steps, trial status, flies, skip: S each][trial row status, re-screen status: n each][ephemeris status S, D]
struct ArWorkspace {
    void *aj, *scr;
    FlightSet f;                      // the constellation itself, not copies: Ks, tf and consts are the caller's (ar_enqueue), read only
    double *du_try, *sat_try, *row_try, *z, *trhs;
    int32_t *sat_st_try, *flies, *skip, *row_st_try, *scr_st, *eph_st, *cat_st;
    size_t bytes;
    ArWorkspace(void *base, int n, int S, int K, int D, int M)
    {
        Carver c(base);
        aj = c.take<char>(AjWorkspace(nullptr, n, S, K).bytes);
        scr = c.take<char>(mpcx_conjunction_pairs_workspace_bytes(S, D, M));       // (the tracked re-screen's is the same size)
        f = FlightSet{};
        f.Ut = c.take<double>((size_t)S * 3 * K);
        f.Yp = c.take<double>((size_t)S * 7 * K);
        f.y0 = c.take<double>((size_t)S * 7);
        f.end_tau = c.take<double>((size_t)S);
        du_try = c.take<double>((size_t)S * 3 * K);
        sat_try = c.take<double>((size_t)S * MPCX_NAJ);
        row_try = c.take<double>((size_t)n * MPCX_NAR);
        z = c.take<double>((size_t)S * AJ_NZ);
        trhs = c.take<double>((size_t)S * 6);
        for (int32_t **q : {&f.pst, &f.nsteps, &sat_st_try, &flies, &skip, &eph_st}) *q = c.take<int32_t>((size_t)S);
        row_st_try = c.take<int32_t>((size_t)n);
        scr_st = c.take<int32_t>((size_t)n);
        cat_st = c.take<int32_t>((size_t)(D > 0 ? D : 1));
        bytes = c.bytes();
    }
};

static int ar_check(mpcx_ctx *ctx, const ArCall &c)
{
    if (int rc = aj_check(ctx, c.j)) return rc;
    if (c.rounds < 0) return ctx_fail(ctx, MPCX_E_BADARG, "avoidance_refine: rounds must be >= 0");
    if (c.M < 2 || !(c.T1 > c.T0)) return ctx_fail(ctx, MPCX_E_BADARG, "avoidance_refine: the re-screen's grid needs M >= 2 and T1 > T0");
    if (!(c.prop_max_step > 0.0)) return ctx_fail(ctx, MPCX_E_BADARG, "avoidance_refine: prop_max_step must be > 0");
    if (c.track && !(c.max_shift == c.max_shift)) return ctx_fail(ctx, MPCX_E_BADARG, "avoidance_refine_tracked: max_shift is NaN");
    if (!c.Y_out || !c.pairs_out || !c.hist_d0 || !c.hist_tca || !c.hist_term || !c.rounds_done)
        return ctx_fail(ctx, MPCX_E_BADARG, "avoidance_refine: Y_out, pairs_out, hist_d0, hist_tca, hist_term and rounds_done are required");
    return MPCX_OK;
}

static int ar_enqueue(mpcx_ctx *ctx, const ArCall &c, void *workspace, hipStream_t st)
{
    const AjCall &j = c.j;
    const int n = j.n, S = j.S, K = j.K, D = j.cat_Y ? j.D : 0;
    ArWorkspace ws(workspace, n, S, K, D, c.M);
    const AjWorkspace aw(ws.aj, n, S, K);
    ws.f.Ks = const_cast<int32_t *>(j.Ks); ws.f.tf = aw.tf; ws.f.consts = const_cast<double *>(j.consts);
    const unsigned gS = (unsigned)((S + 63) / 64), gn = (unsigned)((n + 255) / 256);
    const int most = S * AJ_NZ > n ? S * AJ_NZ : n;
    hipLaunchKernelGGL(ar_init_kernel, dim3((unsigned)((most + 63) / 64)), dim3(64), 0, st, S, K, n, j.Y, j.sat_out, j.sat_status, ws.flies, ws.skip,
                       c.rounds_done, ws.f.y0, ws.f.end_tau, c.hist_term, ws.z, c.rhs_rows, c.rhs_term, 1);
    MPCX_HIP(ctx, hipGetLastError());
    // ---- pass 0: the joint call on what was given
    AjPass first;
    first.z_out = ws.z;
    if (c.rounds == 0) { first.rhs_rows = c.rhs_rows; first.rhs_term = c.rhs_term; }
    if (int rc = aj_enqueue(ctx, j, ws.aj, st, first)) return rc;
    hipLaunchKernelGGL(ar_init_kernel, dim3(gS), dim3(64), 0, st, S, K, n, j.Y, j.sat_out, j.sat_status, ws.flies, ws.skip, c.rounds_done, ws.f.y0,
                       ws.f.end_tau, c.hist_term, ws.z, c.rhs_rows, c.rhs_term, 0);
    MPCX_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(ar_hist_kernel, dim3(gn), dim3(256), 0, st, n, j.row_out, j.pairs, c.hist_d0, c.hist_tca);
    MPCX_HIP(ctx, hipGetLastError());
    for (int t = 1; t <= c.rounds + 1; ++t) {
        const bool solve = t <= c.rounds;
        const size_t total = (size_t)S * 3 * K;
        hipLaunchKernelGGL(ar_apply_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, S, K, j.U, j.du, ws.flies, ws.f.Ut);
        MPCX_HIP(ctx, hipGetLastError());
        if (int rc = ws.f.fly(ctx, S, K, j.flags, c.prop_max_step, st)) return rc;
        hipLaunchKernelGGL(ar_select_kernel, dim3((unsigned)S), dim3(64), 0, st, S, K, j.Ks, j.Y, ws.f.Yp, ws.f.pst, ws.flies, ws.skip, j.sat_status,
                           c.Y_out, c.hist_term + (size_t)t * S);
        MPCX_HIP(ctx, hipGetLastError());
        if (int rc = c.track ? mpcx_conjunction_track_traj_dev(ctx, n, j.pairs, S, K, j.Ks, c.Y_out, j.units, j.span, D, D ? j.cat_K : 0,
                                                               D ? j.cat_Ks : nullptr, D ? j.cat_Y : nullptr, D ? j.cat_units : nullptr,
                                                               D ? j.cat_span : nullptr, c.M, c.T0, c.T1, c.max_shift, c.pairs_out, nullptr,
                                                               ws.scr_st, ws.eph_st, D ? ws.cat_st : nullptr, ws.scr, st)
                             : mpcx_conjunction_pairs_traj_dev(ctx, n, j.pairs, S, K, j.Ks, c.Y_out, j.units, j.span, D, D ? j.cat_K : 0,
                                                               D ? j.cat_Ks : nullptr, D ? j.cat_Y : nullptr, D ? j.cat_units : nullptr,
                                                               D ? j.cat_span : nullptr, c.M, c.T0, c.T1, c.pairs_out, ws.scr_st, ws.eph_st,
                                                               D ? ws.cat_st : nullptr, ws.scr, st))
            return rc;
        AjCall q = j;
        q.pairs = c.pairs_out; q.Y = c.Y_out; q.U = ws.f.Ut;
        q.du = ws.du_try; q.sat_out = ws.sat_try; q.row_out = ws.row_try; q.sat_status = ws.sat_st_try; q.row_status = ws.row_st_try;
        if (!solve) { q.rows = nullptr; q.tsens = nullptr; }
        AjPass x;
        x.solve = solve;
        if (solve) {
            x.uref = j.U; x.z0 = ws.z; x.z_out = ws.z; x.skip = ws.skip; x.trhs = ws.trhs; x.du_prev = j.du; x.Y0 = j.Y;
            if (t == c.rounds) { x.rhs_rows = c.rhs_rows; x.rhs_term = c.rhs_term; }
        }
        if (int rc = aj_enqueue(ctx, q, ws.aj, st, x)) return rc;
        hipLaunchKernelGGL(ar_hist_kernel, dim3(gn), dim3(256), 0, st, n, ws.row_try, c.pairs_out, c.hist_d0 + (size_t)t * n, c.hist_tca + (size_t)t * n);
        MPCX_HIP(ctx, hipGetLastError());
        if (solve) {
            hipLaunchKernelGGL(ar_accept_kernel, dim3((unsigned)S), dim3(64), 0, st, n, K, t, aw.owner, ws.du_try, ws.sat_try, ws.row_try, ws.sat_st_try,
                               ws.row_st_try, ws.skip, j.du, j.sat_out, j.row_out, j.sat_status, j.row_status, c.rounds_done);
            MPCX_HIP(ctx, hipGetLastError());
        }
    }
    return MPCX_OK;
}

}  // namespace mpcx

extern "C" size_t mpcx_avoidance_refine_workspace_bytes(int n, int S, int K, int D, int M)
{
    if (n < 1 || S < 1 || K < 2 || D < 0 || M < 2) return 0;
    return ArWorkspace(nullptr, n, S, K, D, M).bytes;
}

// the arguments of the four entry points below as an ArCall; TRACK, SHIFT: the re-screen's mode
#define MPCX_AR_CALL(TRACK, SHIFT)                                                                                                   \
    ArCall{MPCX_AJ_CALL(0, S), M, T0, T1, prop_max_step, rounds, Y_out, pairs_out, hist_d0, hist_tca, hist_term, rounds_done, rhs_rows, \
           rhs_term, TRACK, SHIFT}

namespace mpcx {

// device pointers throughout in `c`
static int ar_dev(mpcx_ctx *ctx, const ArCall &c, void *workspace, void *stream)
{
    if (int rc = ar_check(ctx, c)) return rc;
    if (!workspace)
        return ctx_fail(ctx, MPCX_E_BADARG, "avoidance_refine: a workspace of mpcx_avoidance_refine_workspace_bytes(n, S, K, D, M) bytes is required");
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    return ar_enqueue(ctx, c, workspace, (hipStream_t)stream);
}

// host pointers throughout in `c`: staged, enqueued, and the results brought back into c's own arrays
static int ar_host(mpcx_ctx *ctx, const ArCall &c)
{
    if (int rc = ar_check(ctx, c)) return rc;
    if (int rc = check_mover(ctx, c.j, c.j.mover, "avoidance_refine")) return rc;
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    DeviceArena ar(ctx);
    ArCall d = c;
    AjCall &j = d.j;
    aj_stage(ar, j, true);
    const int n = c.j.n, S = c.j.S, K = c.j.K;
    const size_t np = (size_t)c.rounds + 2;
    d.Y_out = ar.result(c.Y_out, (size_t)S * 7 * K); d.pairs_out = ar.result(c.pairs_out, (size_t)n * 4);
    d.hist_d0 = ar.result(c.hist_d0, np * n); d.hist_tca = ar.result(c.hist_tca, np * n); d.hist_term = ar.result(c.hist_term, np * S);
    d.rounds_done = ar.result(c.rounds_done, (size_t)S);
    d.rhs_rows = ar.result(c.rhs_rows, (size_t)n);
    d.rhs_term = ar.result(c.rhs_term, (size_t)S * 6);
    return host_run(ctx, ar, mpcx_avoidance_refine_workspace_bytes(n, S, K, c.j.cat_Y ? c.j.D : 0, c.M),
                    [&](void *ws, hipStream_t st) { return ar_enqueue(ctx, d, ws, st); });
}

}  // namespace mpcx

extern "C" int mpcx_avoidance_refine_dev(mpcx_ctx *ctx, int n, const double *pairs, const int32_t *mover, int S, int K, const int32_t *Ks, const
                                         double *Y, const double *U, const double *units, const double *span, const double *consts, int flags,
                                         double max_step, const double *P, int D, int cat_K, const int32_t *cat_Ks, const double *cat_Y, const
                                         double *cat_units, const double *cat_span, const double *cat_P, double mu, double target, const double
                                         *u_max, int hold_terminal, double tol, int max_iter, int M, double T0, double T1, double prop_max_step, int
                                         rounds, double *du, double *sat_out, double *row_out, double *rows, double *tsens, int32_t *sat_status,
                                         int32_t *row_status, double *Y_out, double *pairs_out, double *hist_d0, double *hist_tca, double
                                         *hist_term, int32_t *rounds_done, double *rhs_rows, double *rhs_term, void *workspace, void *stream)
{
    if (!ctx) return MPCX_E_BADARG;
    return ar_dev(ctx, MPCX_AR_CALL(false, 0.0), workspace, stream);
}

extern "C" int mpcx_avoidance_refine(mpcx_ctx *ctx, int n, const double *pairs, const int32_t *mover, int S, int K, const int32_t *Ks, const double
                                     *Y, const double *U, const double *units, const double *span, const double *consts, int flags, double max_step,
                                     const double *P, int D, int cat_K, const int32_t *cat_Ks, const double *cat_Y, const double *cat_units, const
                                     double *cat_span, const double *cat_P, double mu, double target, const double *u_max, int hold_terminal, double
                                     tol, int max_iter, int M, double T0, double T1, double prop_max_step, int rounds, double *du, double *sat_out,
                                     double *row_out, double *rows, double *tsens, int32_t *sat_status, int32_t *row_status, double *Y_out, double
                                     *pairs_out, double *hist_d0, double *hist_tca, double *hist_term, int32_t *rounds_done, double *rhs_rows,
                                     double *rhs_term)
{
    if (!ctx) return MPCX_E_BADARG;
    return ar_host(ctx, MPCX_AR_CALL(false, 0.0));
}

// ---- the same loop with the re-screen that follows each row's own encounter (mpcx_conjunction_track_traj_dev)
extern "C" int mpcx_avoidance_refine_tracked_dev(mpcx_ctx *ctx, int n, const double *pairs, const int32_t *mover, int S, int K, const int32_t *Ks,
                                                 const double *Y, const double *U, const double *units, const double *span, const double *consts,
                                                 int flags, double max_step, const double *P, int D, int cat_K, const int32_t *cat_Ks, const double
                                                 *cat_Y, const double *cat_units, const double *cat_span, const double *cat_P, double mu, double
                                                 target, const double *u_max, int hold_terminal, double tol, int max_iter, int M, double T0, double
                                                 T1, double prop_max_step, int rounds, double max_shift, double *du, double *sat_out, double
                                                 *row_out, double *rows, double *tsens, int32_t *sat_status, int32_t *row_status, double *Y_out,
                                                 double *pairs_out, double *hist_d0, double *hist_tca, double *hist_term, int32_t *rounds_done,
                                                 double *rhs_rows, double *rhs_term, void *workspace, void *stream)
{
    if (!ctx) return MPCX_E_BADARG;
    return ar_dev(ctx, MPCX_AR_CALL(true, max_shift), workspace, stream);
}

extern "C" int mpcx_avoidance_refine_tracked(mpcx_ctx *ctx, int n, const double *pairs, const int32_t *mover, int S, int K, const int32_t *Ks, const
                                             double *Y, const double *U, const double *units, const double *span, const double *consts, int flags,
                                             double max_step, const double *P, int D, int cat_K, const int32_t *cat_Ks, const double *cat_Y, const
                                             double *cat_units, const double *cat_span, const double *cat_P, double mu, double target, const double
                                             *u_max, int hold_terminal, double tol, int max_iter, int M, double T0, double T1, double prop_max_step,
                                             int rounds, double max_shift, double *du, double *sat_out, double *row_out, double *rows, double
                                             *tsens, int32_t *sat_status, int32_t *row_status, double *Y_out, double *pairs_out, double *hist_d0,
                                             double *hist_tca, double *hist_term, int32_t *rounds_done, double *rhs_rows, double *rhs_term)
{
    if (!ctx) return MPCX_E_BADARG;
    return ar_host(ctx, MPCX_AR_CALL(true, max_shift));
}
#undef MPCX_AR_CALL
#undef MPCX_AJ_CALL
