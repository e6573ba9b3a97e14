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
// The window rule's panel loop is stated three times, and a change to the rule is a change to all three:
//   collision_window_kernel               cw_node, cw_rate, the largest rate and its time; a failed node keeps BADK apart from NUMERIC
//   collision_window_sensitivity_kernel   cw_node_at, cw_rate_grad, the gradient scattered to the node sources; the same statuses
//   aw_eval (avoidance_window_device.hpp) cw_node_at, the mean shifted, cw_rate; any failed node is MPCX_ST_NUMERIC
// They call different functions between the same sums and map a failed node to a status differently; one loop for all three would
// need hooks for both, which is more to read than three short loops.  What does not differ is written once
// (collision_window_device.hpp: cw_row, cw_out, cw_out_empty, cw_store), and tests/test_avoidance_window_gpu.py holds the second
// statement to the first one's bytes.
//   collision_window_sensitivity_kernel   the same figure (the same bytes) together with its derivative with respect to every thrust
//                             node of the objects that move (include/mpcx.h: mpcx_collision_window_sensitivity*): the gradient with
//                             respect to the mean relative state at every time node, carried onto the bracketing node states and
//                             swept backwards over the stage records (tests/avoidance_window_reference.py restates it).  Its host
//                             side (cws_check, cws_enqueue: encounter_host.hpp) also serves avoidance_window.hip.
#include "collision_window_device.hpp"
#include "encounter_host.hpp"

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
    double ta = 0.0, tb = 0.0, R = 0.0;
    CpNode na, nb;
    int st = cw_row(a.row, a.col, fi, fj, t, h, ta, tb, R, na, nb);
    if (st == MPCX_ST_OK && !(R > 0.0)) cw_out_empty(o, ta, tb);
    else if (st == MPCX_ST_OK) {
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
                else cw_out(o, total, start, entries, rmax, tmax, ta, tb);
            }
        }
    }
    if (lane == 0) cw_store(o, st, a.out + (size_t)pr * MPCX_NPW, a.status + pr);
}

// the call as both entry points take it
struct CwCall : EncGeometry {
    const double *half;
    int panels;
    double *out;
    int32_t *status;
};
#define MPCX_CW_CALL CwCall{MPCX_GEOMETRY(radius, cat_radius), half_window, panels, out, status}

static int cw_check(mpcx_ctx *ctx, const CwCall &c)
{
    static const char *const name = "collision_probability_window";
    if (int rc = geom_check_sizes(ctx, c, name)) return rc;
    if (c.panels < 1 || c.panels > MPCX_PW_MAX_PANELS) return enc_fail(ctx, name, "panels must be 1..MPCX_PW_MAX_PANELS");
    return geom_check_arrays(ctx, c, name, true, c.half && c.out && c.status, "pairs, Y, units, span, P, radius, half_window, out and status");
}

static int cw_enqueue(mpcx_ctx *ctx, const CwCall &c, hipStream_t st)
{
    CpSide row, col;
    enc_sides(c, row, col);
    const CwArgs a{c.n, c.pairs, row, col, c.mu, c.half, c.panels, c.out, c.status};
    hipLaunchKernelGGL(collision_window_kernel, dim3((unsigned)c.n), dim3(64), 0, st, a);
    MPCX_HIP(ctx, hipGetLastError());
    return MPCX_OK;
}

// ---------------------------------------------------------------- the derivative with respect to the thrust nodes

struct CwsArgs {
    int n, K, NS, who;                // K: the constellation's row length (stage records, sens); NS: slots of sens per row
    const double *pairs;
    CpSide row, col;
    double mu;
    const double *half;
    int panels;
    const double *stage;              // [S][K-1][MPCX_STAGE_DOUBLES]
    const int32_t *dstat;             // the discretiser's status [S]
    double *out, *sens, *sgrad;       // sgrad [n][64 panels + 1][6] or NULL
    double *src;                      // workspace: the node sources [n][2][K][6]
    int32_t *status;
};

enum { CWS_LAM_PAD = 8 };

// One wave per row, lane l time node l of the current panel, as collision_window_kernel -- whose tests and stores this kernel
// shares (cw_row, cw_out) and whose sums it repeats expression for expression: `out` has its bits.  Beside the rate every lane forms c_q (cw_rate_grad) and, for every object
// that moves, what c_q puts on the two node states that bracket its time (cw_basis) into LDS; then lane m - k0 owns node m of the
// panel's nodes k0 .. k1 + 1 and adds the 64 lanes' shares to its source in the order of the lanes.  The ball term is added last.
// The adjoint sweep is avoidance_kernel's: the two half-waves run the two objects side by side, lanes 0..6 of a half own lam, lanes
// 0..2 g_m, a node's record goes through LDS and the next one's is fetched ahead of the arithmetic.
__global__ __launch_bounds__(64) void collision_window_sensitivity_kernel(CwsArgs a)
{
    __shared__ double cb[2][64][12], rec[2][CP_REC_PAD], lam[2][CWS_LAM_PAD];
    __shared__ int kq[2][64];
    const int pr = blockIdx.x, lane = threadIdx.x, h = lane >> 5, ll = lane & 31;
    if (pr >= a.n) return;
    const double *row = a.pairs + (size_t)pr * 4;
    const double fi = row[0], fj = row[1], t = row[3], hw = a.half[pr];
    const size_t K = (size_t)a.K, NQ = (size_t)64 * a.panels + 1;
    double *sens = a.sens + (size_t)pr * a.NS * 3 * K, *src = a.src + (size_t)pr * 2 * K * 6;
    double *sg = a.sgrad ? a.sgrad + (size_t)pr * NQ * 6 : nullptr;
    const bool moves[2] = {a.who != 1, a.NS == 2 && a.who != 0};
    double o[MPCX_NPW];
#pragma unroll
    for (int c = 0; c < MPCX_NPW; ++c) o[c] = cp_nan();
    double ta = 0.0, tb = 0.0, R = 0.0;
    CpNode n0[2];
    int st = cw_row(a.row, a.col, fi, fj, t, hw, ta, tb, R, n0[0], n0[1]);
    const bool empty = st == MPCX_ST_OK && !(R > 0.0);               // no sphere: nothing to differentiate, no mover is looked at
    // the movers' own status counts behind the window rule's (the header's order): it is kept aside until the rule has run
    CpMover mv[2] = {};
    int stm = MPCX_ST_OK;
    if (st == MPCX_ST_OK && !empty) {
#pragma unroll
        for (int sl = 0; sl < 2; ++sl) {
            if (!moves[sl]) continue;
            const int s1 = cp_mover(a.row, a.dstat, n0[sl], K, mv[sl]);
            if (stm == MPCX_ST_OK) stm = s1;
        }
    }
    if (empty) cw_out_empty(o, ta, tb);
    else if (st == MPCX_ST_OK) {
        for (size_t e = lane; e < 2 * K * 6; e += 64) src[e] = 0.0;
        __syncthreads();
        const double ninf = -__longlong_as_double(0x7ff0000000000000LL);
        const double hp = (tb - ta) / (double)a.panels;
        double entries = 0.0, rmax = ninf, tmax = ta;
        int ke[2] = {0, 0};                                          // the last interval a time node falls in, per object
        CwNode nd;
        CpNode nq[2];
        for (int p = 0; p < a.panels && st == MPCX_ST_OK; ++p) {
            const double tau = (ta + (double)p * hp) + (0.5 * hp) * (1.0 + CP_GL[lane][0]);
            const int sl_ = cw_node_at(a.row, a.col, fi, fj, tau, a.mu, nd, nq[0], nq[1]);
            if (__any(sl_ == MPCX_ST_BADK)) st = MPCX_ST_BADK;
            else if (__any(sl_ != MPCX_ST_OK)) st = MPCX_ST_NUMERIC;
            if (st != MPCX_ST_OK) break;
            double cg[6];
            const double rate = cw_rate_grad(nd, R, cg);
            entries = entries + cp_wave_sum(((0.5 * hp) * CP_GL[lane][1]) * rate);
            const double pm = cp_wave_max(rate);
            const double tm = -cp_wave_max(rate == pm ? -tau : ninf);    // the earliest of equal ones
            if (pm > rmax) { rmax = pm; tmax = tm; }
            const double om = (0.5 * hp) * CP_GL[lane][1];
            // c_q; a node where d and w are exactly 0 (the same trajectory twice): the integrand is odd in n, the derivative is 0, and
            // the rule's antipodal points would cancel only to rounding
            const bool still = nd.d[0] == 0.0 && nd.d[1] == 0.0 && nd.d[2] == 0.0 && nd.w[0] == 0.0 && nd.w[1] == 0.0 && nd.w[2] == 0.0;
#pragma unroll
            for (int e = 0; e < 6; ++e) cg[e] = still ? 0.0 : om * cg[e];
            if (sg) {
#pragma unroll
                for (int e = 0; e < 6; ++e) sg[((size_t)p * 64 + lane) * 6 + e] = cg[e];
            }
#pragma unroll
            for (int sl = 0; sl < 2; ++sl) {
                if (!moves[sl]) continue;
                CwBasis b;
                cw_basis(nq[sl], mv[sl].L, a.row.units[2 * mv[sl].o + 1], mv[sl].htau, b);
                const double sgn = sl ? 1.0 : -1.0;
#pragma unroll
                for (int x = 0; x < 4; ++x) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) cb[sl][lane][x * 3 + c] = sgn * (cg[c] * b.p[x] + cg[3 + c] * b.v[x]);
                }
                kq[sl][lane] = nq[sl].k;
            }
            __syncthreads();
#pragma unroll
            for (int sl = 0; sl < 2; ++sl) {
                if (!moves[sl]) continue;
                const int k0 = kq[sl][0], k1 = kq[sl][63];
                ke[sl] = k1;
                for (int m = k0 + lane; m <= k1 + 1; m += 64) {          // (k1 + 1 <= ns - 1 < K)
                    double *sp = src + ((size_t)sl * K + m) * 6;
                    double s[6];
#pragma unroll
                    for (int e = 0; e < 6; ++e) s[e] = sp[e];
                    for (int q = 0; q < 64; ++q) {
                        const int kk = kq[sl][q];
                        if (kk != m && kk + 1 != m) continue;
                        const double *cq = cb[sl][q] + (kk == m ? 0 : 6);
#pragma unroll
                        for (int e = 0; e < 6; ++e) s[e] = s[e] + cq[e];
                    }
#pragma unroll
                    for (int e = 0; e < 6; ++e) sp[e] = s[e];
                }
            }
            __syncthreads();
        }
        if (st == MPCX_ST_OK) {
            st = cw_node_at(a.row, a.col, fi, fj, ta, a.mu, nd, nq[0], nq[1]);      // the same on every lane
            if (st == MPCX_ST_OK) {
                double gz[3], gb[3];
                const double start = nd.cden * cp_wave_sum(cw_ball_share_grad(nd, R, lane, gz));
                const double u0 = cp_wave_sum(gz[0]), u1 = cp_wave_sum(gz[1]), u2 = cp_wave_sum(gz[2]);
                cw_unwhiten(nd, u0, u1, u2, gb);
                const bool centred = nd.d[0] == 0.0 && nd.d[1] == 0.0 && nd.d[2] == 0.0;     // the ball about the mean: 0 by symmetry
#pragma unroll
                for (int c = 0; c < 3; ++c) gb[c] = centred ? 0.0 : nd.cden * gb[c];
                const double total = start + entries;
                if (!cp_finite(total)) st = MPCX_ST_NUMERIC;
                else {
                    cw_out(o, total, start, entries, rmax, tmax, ta, tb);
                    if (lane == 0) {
                        if (sg) {
#pragma unroll
                            for (int c = 0; c < 3; ++c) { sg[(NQ - 1) * 6 + c] = gb[c]; sg[(NQ - 1) * 6 + 3 + c] = 0.0; }
                        }
#pragma unroll
                        for (int sl = 0; sl < 2; ++sl) {
                            if (!moves[sl]) continue;
                            CwBasis b;
                            cw_basis(nq[sl], mv[sl].L, a.row.units[2 * mv[sl].o + 1], mv[sl].htau, b);
                            const double sgn = sl ? 1.0 : -1.0;
                            double *sp = src + ((size_t)sl * K + nq[sl].k) * 6;
#pragma unroll
                            for (int x = 0; x < 4; ++x) {
#pragma unroll
                                for (int c = 0; c < 3; ++c) sp[x * 3 + c] = sp[x * 3 + c] + sgn * (gb[c] * b.p[x]);
                            }
                        }
                    }
                }
            }
        }
        __syncthreads();
        if (st == MPCX_ST_OK && stm != MPCX_ST_OK) {                     // the window rule passed; a mover did not
            st = stm;
#pragma unroll
            for (int c = 0; c < MPCX_NPW; ++c) o[c] = cp_nan();
        }
        if (st == MPCX_ST_OK) {
            // ---- the adjoint sweep: half h of the wave runs the object of slot h
            const bool mine = h < a.NS && moves[h];
            const int kme = h ? ke[1] : ke[0];
            const int kmax = moves[0] ? (moves[1] && ke[1] > ke[0] ? ke[1] : ke[0]) : ke[1];
            const double *srec = a.stage + (size_t)(h ? mv[1].o : mv[0].o) * (K - 1) * MPCX_STAGE_DOUBLES;             // (read only where `mine`)
            const double *sh = src + (size_t)h * K * 6;
            const int lc = ll < 7 ? ll : 0, gc = ll < 3 ? ll : 0;
#pragma unroll
            for (int sl = 0; sl < 2; ++sl) {                             // nodes past ke + 1, and the slot of an object that does not move
                if (sl >= a.NS) continue;
                const int m0 = moves[sl] ? ke[sl] + 2 : 0;
                for (int c = 0; c < 3; ++c)
                    for (int m = m0 + lane; m < a.K; m += 64) sens[((size_t)sl * 3 + c) * K + m] = 0.0;
            }
            if (mine && ll < 7) lam[h][ll] = ll < 6 ? sh[(size_t)(kme + 1) * 6 + ll] : 0.0;           // lam_ke+1 = sigma_ke+1
            double r0 = 0.0, r1 = 0.0, r2 = 0.0;                         // the record in flight: entries ll, ll + 32, ll + 64 (< 91)
            if (mine && kmax <= kme) {
                const double *rp = srec + (size_t)kmax * MPCX_STAGE_DOUBLES;
                r0 = rp[ll]; r1 = rp[ll + 32];
                if (ll + 64 < CP_REC) r2 = rp[ll + 64];
            }
            double carry = 0.0;                                          // lam_q+2 B_kn[q+1], entry gc
            for (int q = kmax; q >= 0; --q) {
                const bool act = mine && q <= kme;
                if (act) {
                    rec[h][ll] = r0; rec[h][ll + 32] = r1;
                    if (ll + 64 < CP_REC) rec[h][ll + 64] = r2;
                }
                __syncthreads();
                if (mine && q >= 1 && q - 1 <= kme) {                    // the next node's record, ahead of this node's arithmetic
                    const double *rp = srec + (size_t)(q - 1) * MPCX_STAGE_DOUBLES;
                    r0 = rp[ll]; r1 = rp[ll + 32];
                    if (ll + 64 < CP_REC) r2 = rp[ll + 64];
                }
                double lnew = 0.0;
                if (act) {
                    lnew = cp_sweep_node(lam[h], rec[h], false, ll < 3, 0, gc, sens + ((size_t)h * 3 + gc) * K + q + 1, carry, ll < 7, 0, lc, 0.0);
                    if (ll < 6) lnew = lnew + sh[(size_t)q * 6 + ll];    // lam_q = lam_q+1 A_q + sigma_q
                }
                __syncthreads();
                if (act && ll < 7) lam[h][ll] = lnew;
            }
            if (mine && ll < 3) sens[((size_t)h * 3 + ll) * K] = carry;  // g_0 = lam_1 B_kn[0]
        }
    }
    if (st != MPCX_ST_OK || empty) {                                     // a failed row is NaN throughout; no sphere: zero
        const double f = empty ? 0.0 : cp_nan();
        for (size_t e = lane; e < (size_t)a.NS * 3 * K; e += 64) sens[e] = f;
        if (sg)
            for (size_t e = lane; e < NQ * 6; e += 64) sg[e] = f;
    }
    if (lane == 0) cw_store(o, st, a.out + (size_t)pr * MPCX_NPW, a.status + pr);
}

int cws_check(mpcx_ctx *ctx, const CwsCall &c, const char *name, bool outputs_given, const char *outputs)
{
    EncProblem p = c;
    p.target = 1.0;                                                  // (not an argument of these calls)
    if (c.cat_Y && (!c.cat_P || !c.cat_radius)) return enc_fail(ctx, name, "cat_P and cat_radius are required with cat_Y");
    if (int rc = enc_check(ctx, p, name, c.P && c.radius && c.half && outputs_given, outputs)) return rc;
    if (c.panels < 1 || c.panels > MPCX_PW_MAX_PANELS) return enc_fail(ctx, name, "panels must be 1..MPCX_PW_MAX_PANELS");
    if (c.who < 0 || c.who > 2) return enc_fail(ctx, name, "who is 0 (object i), 1 (object j) or 2 (both)");
    if (c.cat_Y && c.who != 0) return enc_fail(ctx, name, "only the row object can manoeuvre against a catalogue (who = 0)");
    return MPCX_OK;
}

int cws_enqueue(mpcx_ctx *ctx, const CwsCall &c, const CwsWorkspace &ws, hipStream_t st)
{
    CpSide row, col;
    enc_sides(c, row, col);
    const CwsArgs a{c.n, c.K, c.cat_Y ? 1 : 2, c.who, c.pairs, row, col, c.mu, c.half, c.panels, ws.stage, ws.dstat,
                    c.out, c.sens, c.state_grad, ws.src, c.status};
    hipLaunchKernelGGL(collision_window_sensitivity_kernel, dim3((unsigned)c.n), dim3(64), 0, st, a);
    MPCX_HIP(ctx, hipGetLastError());
    return MPCX_OK;
}

// workspace of the _dev call
struct CwsOwnWorkspace : CwsWorkspace {
    size_t bytes;
    CwsOwnWorkspace(void *base, int n, int S, int K)
    {
        Carver c(base);
        carve_cws(c, n, S, K);
        bytes = c.bytes();
    }
};

static int cws_run(mpcx_ctx *ctx, const CwsCall &c, void *workspace, hipStream_t st)
{
    const CwsOwnWorkspace ws(workspace, c.n, c.S, c.K);
    if (int rc = enc_linearise(ctx, c, ws, st)) return rc;
    return cws_enqueue(ctx, c, ws, st);
}

// the arguments of both entry points as a CwsCall (the target is not an argument of theirs)
#define MPCX_CWS_CALL CwsCall{MPCX_ENC_PROBLEM(radius, cat_radius, 1.0), half_window, panels, who, out, sens, state_grad, status}

static const char *const CWS_NAME = "collision_window_sensitivity";
static const char *const CWS_REQUIRED = "P, radius, half_window, out, sens and status";

}  // namespace mpcx

using namespace mpcx;

extern "C" size_t mpcx_collision_window_sensitivity_workspace_bytes(int n, int S, int K, int panels)
{
    if (n < 1 || S < 1 || K < 2 || panels < 1 || panels > MPCX_PW_MAX_PANELS) return 0;
    return CwsOwnWorkspace(nullptr, n, S, K).bytes;
}

extern "C" int mpcx_collision_window_sensitivity_dev(mpcx_ctx *ctx, int n, const double *pairs, int S, int K, const int32_t *Ks, const double *Y,
                                                     const double *U, const double *units, const double *span, const double *consts,
                                                     int flags, double max_step, const double *P, const double *radius, int D, int cat_K,
                                                     const int32_t *cat_Ks, const double *cat_Y, const double *cat_units,
                                                     const double *cat_span, const double *cat_P, const double *cat_radius, double mu,
                                                     const double *half_window, int panels, int who, double *out, double *sens,
                                                     double *state_grad, int32_t *status, void *workspace, void *stream)
{
    if (!ctx) return MPCX_E_BADARG;
    const CwsCall c = MPCX_CWS_CALL;
    if (int rc = cws_check(ctx, c, CWS_NAME, out && sens && status, CWS_REQUIRED)) return rc;
    if (!workspace)
        return enc_fail(ctx, CWS_NAME, "a workspace of mpcx_collision_window_sensitivity_workspace_bytes(n, S, K, panels) bytes is required");
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    return cws_run(ctx, c, workspace, (hipStream_t)stream);
}

extern "C" int mpcx_collision_window_sensitivity(mpcx_ctx *ctx, int n, const double *pairs, int S, int K, const int32_t *Ks, const double *Y,
                                                 const double *U, const double *units, const double *span, const double *consts, int flags,
                                                 double max_step, const double *P, const double *radius, int D, int cat_K,
                                                 const int32_t *cat_Ks, const double *cat_Y, const double *cat_units, const double *cat_span,
                                                 const double *cat_P, const double *cat_radius, double mu, const double *half_window,
                                                 int panels, int who, double *out, double *sens, double *state_grad, int32_t *status)
{
    if (!ctx) return MPCX_E_BADARG;
    const CwsCall c = MPCX_CWS_CALL;
    if (int rc = cws_check(ctx, c, CWS_NAME, out && sens && status, CWS_REQUIRED)) return rc;
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    DeviceArena ar(ctx);
    CwsCall d = c;
    const size_t NS = cat_Y ? 1 : 2, NQ = (size_t)64 * panels + 1;
    enc_upload(ar, d); d.half = ar.upload(half_window, (size_t)n);
    d.out = ar.result(out, (size_t)n * MPCX_NPW);
    d.sens = ar.result(sens, (size_t)n * NS * 3 * K);
    d.state_grad = ar.result(state_grad, (size_t)n * NQ * 6);
    d.status = ar.result(status, (size_t)n);
    return host_run(ctx, ar, mpcx_collision_window_sensitivity_workspace_bytes(n, S, K, panels),
                    [&](void *ws, hipStream_t st) { return cws_run(ctx, d, ws, st); });
}
#undef MPCX_CWS_CALL

extern "C" int mpcx_collision_probability_window_dev(mpcx_ctx *ctx, int n, const double *pairs, int S, int K, const int32_t *Ks,
                                                     const double *Y, const double *units, const double *span, const double *P,
                                                     const double *radius, int D, int cat_K, const int32_t *cat_Ks, const double *cat_Y,
                                                     const double *cat_units, const double *cat_span, const double *cat_P,
                                                     const double *cat_radius, double mu, const double *half_window, int panels,
                                                     double *out, int32_t *status, void *stream)
{
    if (!ctx) return MPCX_E_BADARG;
    const CwCall c = MPCX_CW_CALL;
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
    const CwCall c = MPCX_CW_CALL;
    if (int rc = cw_check(ctx, c)) return rc;
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    DeviceArena ar(ctx);
    CwCall d = c;
    geom_upload(ar, d); d.half = ar.upload(half_window, (size_t)n);
    d.out = ar.result(out, (size_t)n * MPCX_NPW);
    d.status = ar.result(status, (size_t)n);
    return host_run(ctx, ar, 0, [&](void *, hipStream_t st) { return cw_enqueue(ctx, d, st); });
}
#undef MPCX_CW_CALL
