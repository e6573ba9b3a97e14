// avoidance_window_refine.hip -- the window-probability manoeuvre flown, looked at and corrected again (include/mpcx.h:
// mpcx_avoidance_window_refine*).
//   pass 0            mpcx_avoidance_window as it is (aw_enqueue); awr_first_kernel: who flies, the histories' first entries;
//                     awr_gather_kernel: the virtual constellation -- every row's own copy of its objects, n NS trajectories, the list
//                     re-indexed to (r NS, r NS + 1), against a catalogue to (r, j).  Only rows that passed pass 0 are gathered: their
//                     indices went through cp_state's tests.  A row that failed reads object 0 under NaN indices, which every kernel
//                     below answers with MPCX_ST_BADK before it reads anything.
//   pass t >= 1       awr_apply_kernel    U_t = U + du_t-1 for a row that flies
//                     propagate           every virtual trajectory from its first node under U_t
//                     awr_select_kernel   Y_t: the flight of a slot that moves in a row that flies, the given trajectory otherwise
//                     the time            mpcx_conjunction_track_traj_dev of the list AS GIVEN on Y_t (M >= 2); awr_time_kernel
//                     linearisation about (Y_t, U_t); the covariance chain over its records (recov); awr_pselect_kernel
//                     the figure          mpcx_collision_probability_window_dev on Y_t, P_t at t_t; awr_hist_kernel
//                     the solve           collision_window_sensitivity_kernel (cws_enqueue) on the pass's data, awr_solve_kernel
//   pass rounds + 1   the same without the solve: the answer is returned as flown
// Everything is enqueued on one stream, the number of passes is fixed, nothing is read back in between.  A failure at t >= 1
// freezes the row: it keeps du_t-1, reports the status, is not solved again and keeps flying.
// awr_solve_kernel is avoidance_window_kernel about what was flown, on the same device functions (avoidance_window_device.hpp, with
// a previous response): one wave per row, the direction and Gamma from the pass's sensitivities, two forward chains over the pass's
// stage records (the response to the unit direction e and to du_t-1), the window rule at the means moved by sgn (alpha X_e -
// X_prev), the search from alpha_1 = (c0 + Q_t ln(Q_t / target_p)) / Gamma_t.  No atomics, nothing crosses a workgroup; every sum
// has a fixed order.  tests/avoidance_window_refine_reference.py restates the loop.
#include "avoidance_window_device.hpp"
#include "encounter_host.hpp"

#include <math.h>

namespace mpcx {

// ---------------------------------------------------------------- the bookkeeping kernels

// after pass 0: who flies (never changes afterwards), the histories' first entries
__global__ __launch_bounds__(256) void awr_first_kernel(int n, int rounds, const double *pairs, const double *out, const int32_t *status,
                                                        int32_t *flies, int32_t *frozen, int32_t *ok0, int32_t *rounds_done, double *hist_p,
                                                        double *hist_t, double *hist_pred)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const bool ok = status[r] == MPCX_ST_OK;
    const bool f = ok && out[(size_t)r * MPCX_NAW + MPCX_AW_ALPHA] > 0.0;
    flies[r] = f; frozen[r] = 0; ok0[r] = ok; rounds_done[r] = f ? 0 : -1;
    hist_p[r] = out[(size_t)r * MPCX_NAW + MPCX_AW_P0];
    hist_t[r] = pairs[(size_t)r * 4 + 3];
    for (int t = 0; t <= rounds; ++t) hist_pred[(size_t)t * n + r] = cp_nan();
    if (f) hist_pred[r] = out[(size_t)r * MPCX_NAW + MPCX_AW_P1];
}

struct AwrVirtual {
    FlightSet f;                      // the V virtual trajectories as they fly
    int32_t *obj;                     // [V]: the object a virtual trajectory copies
    double *units, *span, *radius, *q, *P0;
    double *pairs, *pairs_trk;        // [n][4]: the list on the virtual constellation; the same for the tracker (a row whose two
};                                    //   objects are one is no pair to it, as on the given indices)

// One block per virtual trajectory v = r NS + slot.
__global__ __launch_bounds__(64) void awr_gather_kernel(int n, int NS, int S, int K, const double *pairs, const int32_t *ok0, const int32_t *Ks,
                                                        const double *Y, const double *units, const double *span, const double *consts,
                                                        const double *P, const double *radius, const double *q, AwrVirtual w)
{
    const int v = blockIdx.x, lane = threadIdx.x;
    const int r = v / NS, sl = v - r * NS;
    const bool ok = ok0[r] != 0;
    const double *row = pairs + (size_t)r * 4;
    const int o = ok ? (int)row[sl] : 0;                            // (a row that passed pass 0: cp_state tested the index)
    if (lane < 7) w.f.y0[(size_t)v * 7 + lane] = Y[((size_t)o * 7 + lane) * K];
    if (lane < 36) w.P0[(size_t)v * 36 + lane] = P[(size_t)o * K * 36 + lane];
    if (lane < MPCX_NCONST) w.f.consts[(size_t)v * MPCX_NCONST + lane] = consts[(size_t)o * MPCX_NCONST + lane];
    if (lane < 2) { w.units[2 * (size_t)v + lane] = units[2 * (size_t)o + lane]; w.span[2 * (size_t)v + lane] = span[2 * (size_t)o + lane]; }
    if (lane == 0) {
        w.obj[v] = o;
        w.f.Ks[v] = Ks ? Ks[o] : K;
        w.radius[v] = radius[o];
        w.q[v] = q ? q[o] : 0.0;
        double tfv;
        w.f.tf[v] = tr_tf(span[2 * (size_t)o], span[2 * (size_t)o + 1], units[2 * (size_t)o + 1], tfv) ? tfv : 1.0;
        w.f.end_tau[v] = 1.0;
        if (sl == 0) {
            double *pv = w.pairs + (size_t)r * 4, *pt = w.pairs_trk + (size_t)r * 4;
            const double vi = ok ? (double)v : cp_nan();
            const double vj = ok ? (NS == 2 ? (double)(v + 1) : row[1]) : cp_nan();
            const bool one = NS == 2 && row[0] == row[1];
            pv[0] = vi; pv[1] = vj; pv[2] = row[2]; pv[3] = row[3];
            pt[0] = one ? cp_nan() : vi; pt[1] = one ? cp_nan() : vj; pt[2] = row[2]; pt[3] = row[3];
        }
    }
}

__device__ __forceinline__ bool awr_moves(int who, int NS, int sl) { return sl ? (NS == 2 && who != 0) : who != 1; }

__global__ __launch_bounds__(256) void awr_apply_kernel(int V, int NS, int K, const double *U, const double *du, const int32_t *obj,
                                                        const int32_t *flies, double *Ut)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x, per = (size_t)3 * K;
    if (e >= (size_t)V * per) return;
    const size_t v = e / per;
    const double u = U[(size_t)obj[v] * per + (e - v * per)];
    Ut[e] = flies[v / NS] ? u + du[e] : u;
}

// One block per row.  A failed flight freezes the row (the slots in order: slot 0's status first).
__global__ __launch_bounds__(64) void awr_select_kernel(int NS, int K, int who, const double *Y, const double *Yp, const int32_t *pst,
                                                        const int32_t *obj, const int32_t *Ksv, const int32_t *flies, int32_t *frozen,
                                                        int32_t *status, double *Yt)
{
    const int r = blockIdx.x, lane = threadIdx.x;
    const bool fl = flies[r] != 0;
    for (int sl = 0; sl < NS; ++sl) {
        const size_t v = (size_t)r * NS + sl;
        const bool flown = fl && awr_moves(who, NS, sl) && pst[v] == MPCX_ST_OK;
        const int ns = Ksv[v];
        const double *src = flown ? Yp + v * 7 * K : Y + (size_t)obj[v] * 7 * K;
        for (int e = lane; e < 7 * K; e += 64) Yt[v * 7 * K + e] = flown && e % K >= ns ? 0.0 : src[e];
    }
    if (lane == 0 && fl && !frozen[r])
        for (int sl = 0; sl < NS; ++sl) {
            const size_t v = (size_t)r * NS + sl;
            if (awr_moves(who, NS, sl) && pst[v] != MPCX_ST_OK) { frozen[r] = 1; status[r] = pst[v]; break; }
        }
}

// the pass's list: the virtual indices with the pass's time; a row that flies and has lost its event is frozen with MPCX_ST_BADK
__global__ __launch_bounds__(256) void awr_time_kernel(int n, int tracked, const double *pairs_v, const double *trk, const int32_t *flies,
                                                       int32_t *frozen, int32_t *status, double *pairs_t, double *hist_t)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const double *pv = pairs_v + (size_t)r * 4;
    double dist = pv[2], tt = pv[3];
    if (tracked && flies[r]) {
        dist = trk[(size_t)r * 4 + 2]; tt = trk[(size_t)r * 4 + 3];
        if (!cp_finite(tt)) {
            tt = cp_nan();
            if (!frozen[r]) { frozen[r] = 1; status[r] = MPCX_ST_BADK; }
        }
    }
    double *pt = pairs_t + (size_t)r * 4;
    pt[0] = pv[0]; pt[1] = pv[1]; pt[2] = dist; pt[3] = tt;
    hist_t[r] = tt;
}

// One block per row: P_t is the chain's of a slot that moves in a row that flies (chain = 1), the given covariances otherwise
__global__ __launch_bounds__(64) void awr_pselect_kernel(int NS, int K, int who, int chain, const double *P, const double *Pc, const int32_t *cst,
                                                         const int32_t *obj, const int32_t *flies, int32_t *frozen, int32_t *status,
                                                         double *Pt)
{
    const int r = blockIdx.x, lane = threadIdx.x;
    const bool fl = chain && flies[r] != 0;
    for (int sl = 0; sl < NS; ++sl) {
        const size_t v = (size_t)r * NS + sl, per = (size_t)K * 36;
        const double *src = fl && awr_moves(who, NS, sl) ? Pc + v * per : P + (size_t)obj[v] * per;
        for (size_t e = lane; e < per; e += 64) Pt[v * per + e] = src[e];
    }
    if (lane == 0 && fl && !frozen[r])
        for (int sl = 0; sl < NS; ++sl) {
            const size_t v = (size_t)r * NS + sl;
            if (awr_moves(who, NS, sl) && cst[v] != MPCX_ST_OK) { frozen[r] = 1; status[r] = cst[v]; break; }
        }
}

// Q_t of the pass; a row that does not fly repeats pass 0's figure
__global__ __launch_bounds__(256) void awr_hist_kernel(int n, const double *fig, const int32_t *fst, const int32_t *flies, int32_t *frozen,
                                                       int32_t *status, const double *hist0, double *hist_p)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    if (!flies[r]) { hist_p[r] = hist0[r]; return; }
    const int st = fst[r];
    hist_p[r] = st == MPCX_ST_OK ? fig[(size_t)r * MPCX_NPW + MPCX_PW_START] + fig[(size_t)r * MPCX_NPW + MPCX_PW_ENTRIES] : cp_nan();
    if (st != MPCX_ST_OK && !frozen[r]) { frozen[r] = 1; status[r] = st; }
}

// ---------------------------------------------------------------- the solve about what was flown

// the pass's list, the virtual constellation with the pass's trajectories and covariances (and the columns), the pass's
// linearisation [V][K-1][MPCX_STAGE_DOUBLES] with the discretiser's status [V], the sensitivity kernel's answers on the pass's data;
// dx: the responses [n][2 (e, du_t-1)][2][K][6]; out, du, status: the call's own
struct AwrArgs : AwArgs {
    int t;                            // the pass
    double *e;                        // workspace: the unit direction [n][NS][3][K]
    double *sens;                     // the call's own; may be NULL
    const int32_t *flies;
    int32_t *frozen, *rounds_done;
    double *pred;                     // hist_pred of this pass [n]
};

__global__ __launch_bounds__(64) void awr_solve_kernel(AwrArgs a)
{
    __shared__ double rec[2][CP_REC_PAD], xs[2][8];
    const int pr = blockIdx.x, lane = threadIdx.x, h = lane >> 5, ll = lane & 31;
    if (pr >= a.n) return;
    if (!a.flies[pr] || a.frozen[pr]) return;                        // (wave-uniform; frozen is written below by lane 0 at the very end)
    const size_t K = (size_t)a.K, per = (size_t)a.NS * 3 * K;
    const double *g = a.g + (size_t)pr * per, *wo = a.wout + (size_t)pr * MPCX_NPW;
    double *du = a.du + (size_t)pr * per, *e = a.e + (size_t)pr * per, *dx = a.dx + (size_t)pr * 4 * K * 6;
    double *o = a.out + (size_t)pr * MPCX_NAW;
    int st = a.wstat[pr];
    if (a.sens)
        for (size_t m = lane; m < per; m += 64) a.sens[(size_t)pr * per + m] = g[m];
    const double Qt = wo[MPCX_PW_START] + wo[MPCX_PW_ENTRIES];
    if (st == MPCX_ST_OK && (!(Qt > 0.0) || !cp_finite(Qt))) st = MPCX_ST_NUMERIC;       // (no sphere, or a figure that has no logarithm)
    double alpha = 0.0, Q1 = Qt, c0 = 0.0, Gam = 0.0, dv[2] = {0.0, 0.0}, um[2] = {0.0, 0.0};
    int evals = 0;
    bool kept = false;                                               // within tol as flown: du_t-1 is accepted as it is
    if (st == MPCX_ST_OK) {
        const double f0 = log(Qt / a.target);
        if (fabs(f0) <= a.tol) kept = true;
        else {
            AwRow r;
            int ke[2];
            aw_row(a, a.pairs + (size_t)pr * 4, wo, dx, dx + 2 * K * 6, r, ke);
            // ---- the unit direction e (du for alpha = 1) and Gamma_t: the mass row Y_t's
            aw_direction(a, r, g, e, lane, Gam, dv, um);
            // ---- c0 = -sum g_m du_t-1,m in the order slot, node, component (every lane the same sum)
            {
                double s = 0.0;
                for (int sl = 0; sl < a.NS; ++sl)
                    for (int m = 0; m < a.K; ++m)
                        for (int c = 0; c < 3; ++c) s = s + g[((size_t)sl * 3 + c) * K + m] * du[((size_t)sl * 3 + c) * K + m];
                c0 = -s;
            }
            if (!(Gam > 0.0) || !cp_finite(Gam)) st = MPCX_ST_SINGULAR;
            alpha = (c0 + Qt * f0) / Gam;
            if (st == MPCX_ST_OK && (!(alpha > 0.0) || !cp_finite(alpha))) st = MPCX_ST_NUMERIC;
            __syncthreads();                                         // e is read back by other lanes below
            if (st == MPCX_ST_OK) {
                aw_chain(a, r, ke, e, dx, rec, xs, h, ll);
                aw_chain(a, r, ke, du, dx + 2 * K * 6, rec, xs, h, ll);
                // ---- the step: from alpha_1 double until f <= 0 or halve until f > 0, then close the bracket
                double lo = 0.0, flo = 0.0, hi = 0.0, fhi = 0.0;
                bool found = false, bracket = false;
                int dir = 0;                                         // +1: doubling, -1: halving
                while (st == MPCX_ST_OK && !found && !bracket) {     // bracketing
                    if (evals == a.max_eval) { st = MPCX_ST_INFEASIBLE; break; }
                    Q1 = aw_eval<true>(a, r, alpha, lane, st);
                    ++evals;
                    if (st != MPCX_ST_OK) break;
                    if (!(Q1 >= 0.0) || !cp_finite(Q1) || !cp_finite(alpha) || !(alpha > 0.0)) { st = MPCX_ST_NUMERIC; break; }
                    const double f = log(Q1 / a.target);
                    if (fabs(f) <= a.tol) { found = true; break; }
                    if (f > 0.0) {
                        lo = alpha; flo = f;
                        if (dir < 0) { bracket = true; break; }
                        dir = 1;
                        alpha = 2.0 * alpha;
                    } else {
                        hi = alpha; fhi = f;
                        if (dir > 0) { bracket = true; break; }
                        dir = -1;
                        alpha = 0.5 * alpha;
                    }
                }
                aw_close<true>(a, r, lane, lo, flo, hi, fhi, found, alpha, Q1, evals, st);
                if (st == MPCX_ST_OK) {                              // accepted: du = alpha e, the total change from the given U
#pragma unroll
                    for (int sl = 0; sl < 2; ++sl) {
                        if (sl >= a.NS) continue;
                        for (int c = 0; c < 3; ++c)
                            for (int m = lane; m < a.K; m += 64) du[((size_t)sl * 3 + c) * K + m] = alpha * e[((size_t)sl * 3 + c) * K + m];
                    }
                }
            }
        }
    }
    if (lane == 0) {
        o[MPCX_AW_EVALS] = o[MPCX_AW_EVALS] + (double)evals;
        if (st != MPCX_ST_OK) { a.status[pr] = st; a.frozen[pr] = 1; }
        else {
            o[MPCX_AW_P1] = Q1;
            if (!kept) {
                o[MPCX_AW_ALPHA] = alpha; o[MPCX_AW_DQ_LINEAR] = c0 - alpha * Gam;
                o[MPCX_AW_DV_I] = alpha * dv[0]; o[MPCX_AW_DV_J] = alpha * dv[1];
                o[MPCX_AW_UMAX_I] = alpha * um[0]; o[MPCX_AW_UMAX_J] = alpha * um[1];
            }
            a.rounds_done[pr] = a.t;
            a.pred[pr] = Q1;
        }
    }
}

// ---------------------------------------------------------------- the host side

struct AwrCall {
    AwCall w;
    double prop_max_step;
    int rounds, M;
    double T0, T1, max_shift;
    int recov;
    const double *q;
    int32_t *rounds_done;
    double *Y_out, *P_out, *hist_p, *hist_t, *hist_pred;
};

static const char *const AWR_NAME = "avoidance_window_refine";

static int awr_check(mpcx_ctx *ctx, const AwrCall &c)
{
    if (int rc = aw_check(ctx, c.w, AWR_NAME)) return rc;
    if (!(c.prop_max_step > 0.0)) return enc_fail(ctx, AWR_NAME, "prop_max_step must be > 0");
    if (c.rounds < 0) return enc_fail(ctx, AWR_NAME, "rounds must be >= 0");
    if (c.M < 0 || c.M == 1) return enc_fail(ctx, AWR_NAME, "M is 0 (every row keeps its given time) or >= 2 (the tracker's grid)");
    if (c.M >= 2 && !(c.T1 > c.T0)) return enc_fail(ctx, AWR_NAME, "the tracker's grid needs T1 > T0");
    if (c.M >= 2 && !(c.max_shift == c.max_shift)) return enc_fail(ctx, AWR_NAME, "max_shift is NaN");
    if (c.recov < 0 || c.recov > 1) return enc_fail(ctx, AWR_NAME, "recov is 0 or 1");
    if (!c.rounds_done || !c.Y_out || !c.hist_p || !c.hist_t || !c.hist_pred)
        return enc_fail(ctx, AWR_NAME, "rounds_done, Y_out, hist_p, hist_t and hist_pred are required");
    return MPCX_OK;
}

// [pass 0's workspace][the tracker's][the virtual constellation][U_t, flight, chain's P, P_t: V rows][the pass's linearisation and node
// sources][the pass's figure, sensitivities, direction, responses: n rows][statuses]
struct AwrWorkspace {
    void *aw, *scr;
    AwrVirtual v;
    double *Pc, *Pt, *trk, *pairs_t, *fig, *wout, *g, *e, *dx;
    CwsWorkspace lin;
    int32_t *cst, *eph_st, *cat_st, *trk_st, *fst, *wstat, *flies, *frozen, *ok0;
    size_t bytes;
    AwrWorkspace(void *base, int n, int S, int K, int D, int M, int panels, int NS)
    {
        const size_t V = (size_t)n * NS;
        Carver c(base);
        aw = c.take<char>(mpcx_avoidance_window_workspace_bytes(n, S, K, panels));
        scr = c.take<char>(M >= 2 ? mpcx_conjunction_track_workspace_bytes((int)V, D, M) : 0);
        v.f.carve(c, V, (size_t)K);
        v.obj = c.take<int32_t>(V);
        v.units = c.take<double>(V * 2); v.span = c.take<double>(V * 2);
        v.radius = c.take<double>(V); v.q = c.take<double>(V); v.P0 = c.take<double>(V * 36);
        v.pairs = c.take<double>((size_t)n * 4); v.pairs_trk = c.take<double>((size_t)n * 4);
        Pc = c.take<double>(V * K * 36); Pt = c.take<double>(V * K * 36);
        trk = c.take<double>((size_t)n * 4); pairs_t = c.take<double>((size_t)n * 4);
        lin.carve_cws(c, n, (int)V, K);
        fig = c.take<double>((size_t)n * MPCX_NPW); wout = c.take<double>((size_t)n * MPCX_NPW);
        g = c.take<double>((size_t)n * 2 * 3 * K); e = c.take<double>((size_t)n * 2 * 3 * K);
        dx = c.take<double>((size_t)n * 4 * K * 6);
        for (int32_t **p : {&cst, &eph_st}) *p = c.take<int32_t>(V);
        cat_st = c.take<int32_t>((size_t)(D > 0 ? D : 1));
        for (int32_t **p : {&trk_st, &fst, &wstat, &flies, &frozen, &ok0}) *p = c.take<int32_t>((size_t)n);
        bytes = c.bytes();
    }
};

// device pointers throughout in `c`
static int awr_enqueue(mpcx_ctx *ctx, const AwrCall &c, void *workspace, hipStream_t st)
{
    const AwCall &w = c.w;
    const int n = w.n, S = w.S, K = w.K, NS = w.cat_Y ? 1 : 2, D = w.cat_Y ? w.D : 0, V = n * NS;
    const AwrWorkspace ws(workspace, n, S, K, D, c.M, w.panels, NS);
    const unsigned gn = (unsigned)((n + 255) / 256);
    const size_t np = (size_t)n;
    // ---- pass 0: the window manoeuvre on what was given
    if (int rc = aw_enqueue(ctx, w, ws.aw, st)) return rc;
    hipLaunchKernelGGL(awr_first_kernel, dim3(gn), dim3(256), 0, st, n, c.rounds, w.pairs, w.out, w.status, ws.flies, ws.frozen, ws.ok0,
                       c.rounds_done, c.hist_p, c.hist_t, c.hist_pred);
    MPCX_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(awr_gather_kernel, dim3((unsigned)V), dim3(64), 0, st, n, NS, S, K, w.pairs, ws.ok0, w.Ks, w.Y, w.units, w.span, w.consts,
                       w.P, w.radius, c.recov ? c.q : nullptr, ws.v);
    MPCX_HIP(ctx, hipGetLastError());
    double *Pt = c.recov ? (c.P_out ? c.P_out : ws.Pt) : nullptr;
    for (int t = 1; t <= c.rounds + 1; ++t) {
        const bool solve = t <= c.rounds;
        const size_t total = (size_t)V * 3 * K;
        hipLaunchKernelGGL(awr_apply_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, V, NS, K, w.U, w.du, ws.v.obj, ws.flies, ws.v.f.Ut);
        MPCX_HIP(ctx, hipGetLastError());
        if (int rc = ws.v.f.fly(ctx, V, K, w.flags, c.prop_max_step, st)) return rc;
        hipLaunchKernelGGL(awr_select_kernel, dim3((unsigned)n), dim3(64), 0, st, NS, K, w.who, w.Y, ws.v.f.Yp, ws.v.f.pst, ws.v.obj, ws.v.f.Ks, ws.flies,
                           ws.frozen, w.status, c.Y_out);
        MPCX_HIP(ctx, hipGetLastError());
        if (c.M >= 2)
            if (int rc = mpcx_conjunction_track_traj_dev(ctx, n, ws.v.pairs_trk, V, K, ws.v.f.Ks, c.Y_out, ws.v.units, ws.v.span, D, D ? w.cat_K : 0,
                                                         D ? w.cat_Ks : nullptr, D ? w.cat_Y : nullptr, D ? w.cat_units : nullptr,
                                                         D ? w.cat_span : nullptr, c.M, c.T0, c.T1, c.max_shift, ws.trk, nullptr, ws.trk_st,
                                                         ws.eph_st, D ? ws.cat_st : nullptr, ws.scr, st))
                return rc;
        hipLaunchKernelGGL(awr_time_kernel, dim3(gn), dim3(256), 0, st, n, c.M >= 2 ? 1 : 0, ws.v.pairs, ws.trk, ws.flies, ws.frozen, w.status,
                           ws.pairs_t, c.hist_t + (size_t)t * np);
        MPCX_HIP(ctx, hipGetLastError());
        // the pass's problem: the virtual constellation as flown
        CwsCall q = w;
        q.pairs = ws.pairs_t; q.S = V; q.Ks = ws.v.f.Ks; q.Y = c.Y_out; q.U = ws.v.f.Ut; q.units = ws.v.units; q.span = ws.v.span;
        q.consts = ws.v.f.consts; q.radius = ws.v.radius;
        if (solve || c.recov)
            if (int rc = enc_linearise(ctx, q, ws.lin, st)) return rc;
        if (c.recov) {
            if (int rc = cov_enqueue(ctx, V, K, ws.v.f.Ks, ws.lin.stage, ws.lin.dstat, ws.v.units, ws.v.span, ws.v.P0, ws.v.q, ws.Pc, ws.cst, st))
                return rc;
            hipLaunchKernelGGL(awr_pselect_kernel, dim3((unsigned)n), dim3(64), 0, st, NS, K, w.who, 1, w.P, ws.Pc, ws.cst, ws.v.obj, ws.flies, ws.frozen,
                               w.status, Pt);
            MPCX_HIP(ctx, hipGetLastError());
            q.P = Pt;
        } else if (t == 1) {                                         // the given covariances, row for row: they do not change
            hipLaunchKernelGGL(awr_pselect_kernel, dim3((unsigned)n), dim3(64), 0, st, NS, K, w.who, 0, w.P, ws.Pc, ws.cst, ws.v.obj, ws.flies, ws.frozen,
                               w.status, ws.Pt);
            MPCX_HIP(ctx, hipGetLastError());
        }
        if (!c.recov) q.P = ws.Pt;
        if (int rc = mpcx_collision_probability_window_dev(ctx, n, q.pairs, V, K, q.Ks, q.Y, q.units, q.span, q.P, q.radius, D, D ? w.cat_K : 0,
                                                           D ? w.cat_Ks : nullptr, D ? w.cat_Y : nullptr, D ? w.cat_units : nullptr,
                                                           D ? w.cat_span : nullptr, D ? w.cat_P : nullptr, D ? w.cat_radius : nullptr, w.mu,
                                                           w.half, w.panels, ws.fig, ws.fst, st))
            return rc;
        hipLaunchKernelGGL(awr_hist_kernel, dim3(gn), dim3(256), 0, st, n, ws.fig, ws.fst, ws.flies, ws.frozen, w.status, c.hist_p,
                           c.hist_p + (size_t)t * np);
        MPCX_HIP(ctx, hipGetLastError());
        if (!solve) continue;
        q.out = ws.wout; q.status = ws.wstat; q.sens = ws.g; q.state_grad = nullptr;
        if (int rc = cws_enqueue(ctx, q, ws.lin, st)) return rc;
        CpSide row, col;
        enc_sides(q, row, col);
        const AwrArgs a{{n, K, NS, w.who, ws.pairs_t, row, col, w.mu, w.panels, ws.lin.stage, ws.lin.dstat, w.target, w.tol, w.max_eval,
                         ws.wout, ws.wstat, ws.g, ws.dx, w.out, w.du, w.status},
                        t, ws.e, w.sens, ws.flies, ws.frozen, c.rounds_done, c.hist_pred + (size_t)t * np};
        hipLaunchKernelGGL(awr_solve_kernel, dim3((unsigned)n), dim3(64), 0, st, a);
        MPCX_HIP(ctx, hipGetLastError());
    }
    return MPCX_OK;
}

}  // namespace mpcx

using namespace mpcx;

extern "C" size_t mpcx_avoidance_window_refine_workspace_bytes(int n, int S, int K, int D, int M, int panels)
{
    if (n < 1 || S < 1 || K < 2 || D < 0 || M == 1 || M < 0 || panels < 1 || panels > MPCX_PW_MAX_PANELS) return 0;
    return AwrWorkspace(nullptr, n, S, K, D, M, panels, D > 0 ? 1 : 2).bytes;
}

// the arguments of the two entry points below as an AwrCall
#define MPCX_AWR_CALL                                                                                                                         \
    AwrCall{MPCX_AW_CALL, prop_max_step, rounds, M, T0, T1, max_shift, recov, q, rounds_done, Y_out, P_out, hist_p, hist_t, hist_pred}

extern "C" int mpcx_avoidance_window_refine_dev(mpcx_ctx *ctx, int n, const double *pairs, int S, int K, const int32_t *Ks, const double *Y,
                                                const double *U, const double *units, const double *span, const double *consts, int flags,
                                                double max_step, const double *P, const double *radius, int D, int cat_K,
                                                const int32_t *cat_Ks, const double *cat_Y, const double *cat_units, const double *cat_span,
                                                const double *cat_P, const double *cat_radius, double mu, const double *half_window,
                                                int panels, int who, double target_p, double tol, int max_eval, double prop_max_step,
                                                int rounds, int M, double T0, double T1, double max_shift, int recov, const double *q,
                                                double *out, double *du, double *sens, int32_t *status, int32_t *rounds_done, double *Y_out,
                                                double *P_out, double *hist_p, double *hist_t, double *hist_pred, void *workspace,
                                                void *stream)
{
    if (!ctx) return MPCX_E_BADARG;
    const AwrCall c = MPCX_AWR_CALL;
    if (int rc = awr_check(ctx, c)) return rc;
    if (!workspace)
        return enc_fail(ctx, AWR_NAME, "a workspace of mpcx_avoidance_window_refine_workspace_bytes(n, S, K, D, M, panels) bytes is required");
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    return awr_enqueue(ctx, c, workspace, (hipStream_t)stream);
}

extern "C" int mpcx_avoidance_window_refine(mpcx_ctx *ctx, int n, const double *pairs, int S, int K, const int32_t *Ks, const double *Y,
                                            const double *U, const double *units, const double *span, const double *consts, int flags,
                                            double max_step, const double *P, const double *radius, int D, int cat_K, const int32_t *cat_Ks,
                                            const double *cat_Y, const double *cat_units, const double *cat_span, const double *cat_P,
                                            const double *cat_radius, double mu, const double *half_window, int panels, int who,
                                            double target_p, double tol, int max_eval, double prop_max_step, int rounds, int M, double T0,
                                            double T1, double max_shift, int recov, const double *q, double *out, double *du, double *sens,
                                            int32_t *status, int32_t *rounds_done, double *Y_out, double *P_out, double *hist_p,
                                            double *hist_t, double *hist_pred)
{
    if (!ctx) return MPCX_E_BADARG;
    const AwrCall c = MPCX_AWR_CALL;
    if (int rc = awr_check(ctx, c)) return rc;
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    DeviceArena ar(ctx);
    AwrCall d = c;
    const size_t NS = cat_Y ? 1 : 2, V = (size_t)n * NS, np = (size_t)rounds + 2;
    enc_upload(ar, d.w); d.w.half = ar.upload(half_window, (size_t)n);
    d.q = recov && q ? ar.upload(q, (size_t)S) : nullptr;
    d.w.out = ar.result(out, (size_t)n * MPCX_NAW);
    d.w.du = ar.result(du, V * 3 * K);
    d.w.sens = ar.result(sens, V * 3 * K);
    d.w.status = ar.result(status, (size_t)n);
    d.rounds_done = ar.result(rounds_done, (size_t)n);
    d.Y_out = ar.result(Y_out, V * 7 * K);
    d.P_out = ar.result(recov ? P_out : nullptr, V * K * 36);
    d.hist_p = ar.result(hist_p, np * n); d.hist_t = ar.result(hist_t, np * n); d.hist_pred = ar.result(hist_pred, (np - 1) * n);
    return host_run(ctx, ar, mpcx_avoidance_window_refine_workspace_bytes(n, S, K, cat_Y ? D : 0, M, panels),
                    [&](void *ws, hipStream_t st) { return awr_enqueue(ctx, d, ws, st); });
}
#undef MPCX_AWR_CALL
