// avoidance.hip -- from a screen's pairs list to avoidance manoeuvres (include/mpcx.h: mpcx_avoidance*).
//   avoidance_kernel   for every listed pair: the encounter frame at the pair's time of closest approach, a backward (adjoint) sweep
//                      over the stage records the discretiser integrates anyway -- A and, this time, the two first-order-hold input
//                      blocks -- that gives the derivative of the encounter-plane miss with respect to every thrust node of the plan,
//                      and from it the least-effort thrust change that opens the miss to the requested distance.
// One wave per pair.  The sweep is a chain of 3 x 7 by 7 x 7 products, k + 1 of them: the two half-waves run the two objects of a
// pair side by side, lanes 0..20 of a half own the entries of lam, lanes 0..8 those of g_m; a node's A | B_kn | B_kp (the first 91
// doubles of its record) is fetched by the half in one pass of three loads per lane, the next node's before the arithmetic of this
// one.  Everything else is wave-uniform setup or a lane-strided pass over the nodes closed by an xor butterfly: the operation order
// is fixed (tests/avoidance_reference.py restates it), nothing depends on the launch.  LDS: two records and two lam, whatever K.
// The frame, the encounter-plane covariance, the movers' setup, the sweep's seeds and its node step are collision_device.hpp's, where
// collision.hip and avoidance_joint.hip take them from too; this file keeps the sweep's two-half-wave loop and the manoeuvre.
#include "collision_device.hpp"
#include "encounter_host.hpp"

namespace mpcx {

struct AvArgs {
    int n, K, NS, who;                // K: the constellation's row length (stage records, du, sens); NS: slots of du and sens per pair
    const double *pairs;
    CpSide row, col;
    int have_P;
    const double *stage;              // [S][K-1][MPCX_STAGE_DOUBLES]
    const int32_t *dstat;             // the discretiser's status [S]
    double mu, target;
    double *out, *du, *g;             // g [n][NS][3][3][K]: sens when the caller gave it, otherwise the workspace
    int zero_g;                       // g is sens: the nodes the sweep does not reach are part of the result
    int32_t *status;
};

enum { AV_LAM = 21, AV_LAM_PAD = 24 };

// effort-scaled encounter-plane rows of node m of the mover in slot `slot`, its trapezoid weight and c_m; also the raw e_w row
__device__ __forceinline__ void av_node(const CpMover &mv, int slot, const double *g, size_t K, int m, double (&gh)[2][3], double (&gw)[3],
                                        double &wm, double &cm)
{
    cm = mv.cfac / mv.mass[m];
    wm = (m == 0 || m == mv.nn - 1) ? 0.5 * mv.hn : mv.hn;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        gh[0][c] = g[((size_t)slot * 9 + c) * K + m] / cm;
        gh[1][c] = g[((size_t)slot * 9 + 3 + c) * K + m] / cm;
        gw[c] = g[((size_t)slot * 9 + 6 + c) * K + m];
    }
}

__global__ __launch_bounds__(64) void avoidance_kernel(AvArgs a)
{
    __shared__ double rec[2][CP_REC_PAD], lam[2][AV_LAM_PAD];
    const int pr = blockIdx.x, lane = threadIdx.x, h = lane >> 5, ll = lane & 31;
    if (pr >= a.n) return;
    const double *row = a.pairs + (size_t)pr * 4;
    const double t = row[3];
    const size_t K = (size_t)a.K;
    double *du = a.du + (size_t)pr * a.NS * 3 * K, *g = a.g + (size_t)pr * a.NS * 9 * K;
    double o[MPCX_NAV];
#pragma unroll
    for (int c = 0; c < MPCX_NAV; ++c) o[c] = cp_nan();
    const bool moves[2] = {a.who != 1, a.NS == 2 && a.who != 0};

    // ---- both objects at t, the statuses that end the row, the encounter frame and the target's metric (wave-uniform)
    double pa[3], va[3], pb[3], vb[3];
    CpNode nda, ndb;
    int st = cp_state(a.row, row[0], t, pa, va, nda);
    if (st == MPCX_ST_OK) st = cp_state(a.col, row[1], t, pb, vb, ndb);
    CpMover mv[2] = {};
    if (st == MPCX_ST_OK) {
#pragma unroll
        for (int sl = 0; sl < 2; ++sl) {
            if (!moves[sl] || st != MPCX_ST_OK) continue;
            st = cp_mover(a.row, a.dstat, sl ? ndb : nda, K, mv[sl]);
        }
    }
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

    if (st == MPCX_ST_OK) {
        // ---- the adjoint sweep: half h of the wave runs the object of slot h
        const bool mine = h < a.NS && moves[h];
        const int kme = h ? mv[1].k : mv[0].k;
        const int kmax = moves[0] ? (moves[1] && mv[1].k > mv[0].k ? mv[1].k : mv[0].k) : mv[1].k;
        const double *srec = a.stage + (size_t)(h ? ndb.o : nda.o) * (K - 1) * MPCX_STAGE_DOUBLES;     // (read only where `mine`)
        const int lr = ll < AV_LAM ? ll / 7 : 0, lc = ll < AV_LAM ? ll - 7 * (ll / 7) : 0;             // entry of lam
        const int gr = ll < 9 ? ll / 3 : 0, gc = ll < 9 ? ll - 3 * (ll / 3) : 0;                       // entry of g_m
        double seed_hi = 0.0, seed_lo = 0.0;                         // R Lam of the two bracketing nodes, entry (lr, lc)
        {
            const CpNode &nd = h ? ndb : nda;
            cp_sweep_seed(h ? 1.0 : -1.0, e1, e2, ew, h ? mv[1].L : mv[0].L, h ? mv[1].htau : mv[0].htau, nd.h00, nd.h10, nd.h01, nd.h11, lr, lc,
                          seed_hi, seed_lo);
        }
        if (a.zero_g) {                                              // nodes past k + 1, and the slot of an object that does not move
#pragma unroll
            for (int sl = 0; sl < 2; ++sl) {
                if (sl >= a.NS) continue;
                const int m0 = moves[sl] ? mv[sl].k + 2 : 0;
                for (int e = 0; e < 9; ++e)
                    for (int m = m0 + lane; m < a.K; m += 64) g[((size_t)sl * 9 + e) * K + m] = 0.0;
            }
        }
        if (mine && ll < AV_LAM) lam[h][ll] = seed_hi;               // lam_k+1
        double r0 = 0.0, r1 = 0.0, r2 = 0.0;                         // the record in flight: entries ll, ll + 32, ll + 64 (< 91)
        if (mine && kmax <= kme) {
            const double *rp = srec + (size_t)kmax * MPCX_STAGE_DOUBLES;
            r0 = rp[ll]; r1 = rp[ll + 32];
            if (ll + 64 < CP_REC) r2 = rp[ll + 64];
        }
        double carry = 0.0;                                          // lam_q+2 B_kn[q+1], entry (gr, gc)
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
            if (act)
                lnew = cp_sweep_node(lam[h], rec[h], q == kme, ll < 9, gr, gc, g + ((size_t)h * 9 + ll) * K + q + 1, carry, ll < AV_LAM, lr, lc, seed_lo);
            __syncthreads();
            if (act && ll < AV_LAM) lam[h][ll] = lnew;               // lam_q
        }
        if (mine && ll < 9) g[((size_t)h * 9 + ll) * K] = carry;     // g_0 = lam_1 B_kn[0]
        __syncthreads();                                             // g is read back by other lanes below

        // ---- the authority matrix M = sum over movers and nodes of ghat ghat^T / w
        double M11 = 0.0, M12 = 0.0, M22 = 0.0;
#pragma unroll
        for (int sl = 0; sl < 2; ++sl) {
            if (!moves[sl]) continue;
            double s11 = 0.0, s12 = 0.0, s22 = 0.0;
            for (int m = lane; m <= mv[sl].k + 1; m += 64) {
                double gh[2][3], gw[3], wm, cm;
                av_node(mv[sl], sl, g, K, m, gh, gw, wm, cm);
                s11 = s11 + (gh[0][0] * gh[0][0] + gh[0][1] * gh[0][1] + gh[0][2] * gh[0][2]) / wm;
                s12 = s12 + (gh[0][0] * gh[1][0] + gh[0][1] * gh[1][1] + gh[0][2] * gh[1][2]) / wm;
                s22 = s22 + (gh[1][0] * gh[1][0] + gh[1][1] * gh[1][1] + gh[1][2] * gh[1][2]) / wm;
            }
            M11 = M11 + cp_wave_sum(s11); M12 = M12 + cp_wave_sum(s12); M22 = M22 + cp_wave_sum(s22);
        }
        const double detM = M11 * M22 - M12 * M12;
        if (!(detM > 0.0) || !cp_finite(detM) || !cp_finite(M11) || !cp_finite(M22)) st = MPCX_ST_SINGULAR;
        else {
            // ---- the manoeuvre: m = (|m|, 0) in the frame
            const double d0 = sqrt(mn * W11 * mn);
            double dm1 = 0.0, dm2 = 0.0, l1 = 0.0, l2 = 0.0;
            const bool act = d0 < a.target;
            if (act) {
                const double p1 = M11 * W11 + M12 * W12, p2 = M12 * W11 + M22 * W12;           // p = M W (1, 0)^T
                const double Wp1 = W11 * p1 + W12 * p2, Wp2 = W12 * p1 + W22 * p2;
                const double qa = p1 * Wp1 + p2 * Wp2, qb = mn * Wp1, qc = mn * W11 * mn - a.target * a.target;
                const double alpha = -qc / (qb + sqrt(qb * qb - qa * qc));
                dm1 = alpha * p1; dm2 = alpha * p2;
                l1 = (M22 * dm1 - M12 * dm2) / detM; l2 = (M11 * dm2 - M12 * dm1) / detM;      // lambda = M^-1 dm
            }
            double dv[2] = {0.0, 0.0}, um[2] = {0.0, 0.0}, along = 0.0;
#pragma unroll
            for (int sl = 0; sl < 2; ++sl) {
                if (sl >= a.NS) continue;
                const int m0 = moves[sl] && act ? mv[sl].k + 2 : 0;
                for (int c = 0; c < 3; ++c)
                    for (int m = m0 + lane; m < a.K; m += 64) du[((size_t)sl * 3 + c) * K + m] = 0.0;
                if (m0 == 0) continue;
                double sdv = 0.0, sum = 0.0, sal = 0.0;
                for (int m = lane; m <= mv[sl].k + 1; m += 64) {
                    double gh[2][3], gw[3], wm, cm, da[3], dn[3];
                    av_node(mv[sl], sl, g, K, m, gh, gw, wm, cm);
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        da[c] = (gh[0][c] * l1 + gh[1][c] * l2) / wm;
                        dn[c] = da[c] / cm;
                        du[((size_t)sl * 3 + c) * K + m] = dn[c];
                    }
                    sdv = sdv + wm * sqrt(da[0] * da[0] + da[1] * da[1] + da[2] * da[2]);
                    sum = fmax(sum, sqrt(dn[0] * dn[0] + dn[1] * dn[1] + dn[2] * dn[2]));
                    sal = sal + (gw[0] * dn[0] + gw[1] * dn[1] + gw[2] * dn[2]);
                }
                dv[sl] = cp_wave_sum(sdv); um[sl] = cp_wave_max(sum);
                along = along + cp_wave_sum(sal);
            }
            const double x1 = mn + dm1;
            o[MPCX_AV_D0] = d0;
            o[MPCX_AV_D1] = act ? sqrt(x1 * (W11 * x1 + W12 * dm2) + dm2 * (W12 * x1 + W22 * dm2)) : d0;
            o[MPCX_AV_DM1] = dm1; o[MPCX_AV_DM2] = dm2;
            o[MPCX_AV_MISS1] = sqrt(x1 * x1 + dm2 * dm2);
            o[MPCX_AV_DT] = act ? -along / wn : 0.0;
            o[MPCX_AV_DV_I] = dv[0]; o[MPCX_AV_DV_J] = dv[1];
            o[MPCX_AV_UMAX_I] = um[0]; o[MPCX_AV_UMAX_J] = um[1];
        }
    }
    if (st != MPCX_ST_OK) {                                          // a failed row is NaN throughout
        for (size_t e = lane; e < (size_t)a.NS * 3 * K; e += 64) du[e] = cp_nan();
        if (a.zero_g)
            for (size_t e = lane; e < (size_t)a.NS * 9 * K; e += 64) g[e] = cp_nan();
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < MPCX_NAV; ++c) a.out[(size_t)pr * MPCX_NAV + c] = o[c];
        a.status[pr] = st;
    }
}

// workspace of the _dev call: [the linearisation's][g n 2 3 3 K]
struct AvWorkspace : LinWorkspace {
    double *g;
    size_t bytes;
    AvWorkspace(void *base, int n, int S, int K)
    {
        Carver c(base);
        carve(c, S, K);
        g = c.take<double>((size_t)n * 2 * 9 * K);
        bytes = c.bytes();
    }
};

struct AvCall : EncProblem {
    int who;
    double *out, *du, *sens;
    int32_t *status;
};

// the arguments of both entry points as an AvCall
#define MPCX_AV_CALL AvCall{MPCX_ENC_PROBLEM(nullptr, nullptr, target), who, out, du, sens, status}

static int av_check(mpcx_ctx *ctx, const AvCall &c)
{
    if (int rc = enc_check(ctx, c, "avoidance", c.out && c.du && c.status, "out, du and status")) return rc;
    if (c.who < 0 || c.who > 2) return enc_fail(ctx, "avoidance", "who is 0 (object i), 1 (object j) or 2 (both)");
    if (c.cat_Y && c.who != 0) return enc_fail(ctx, "avoidance", "only the row object can manoeuvre against a catalogue (who = 0)");
    return MPCX_OK;
}

static int av_enqueue(mpcx_ctx *ctx, const AvCall &c, void *workspace, hipStream_t st)
{
    const AvWorkspace ws(workspace, c.n, c.S, c.K);
    if (int rc = enc_linearise(ctx, c, ws, st)) return rc;
    CpSide row, col;
    enc_sides(c, row, col);
    const AvArgs a{c.n, c.K, c.cat_Y ? 1 : 2, c.who, c.pairs, row, col, c.P != nullptr, ws.stage, ws.dstat, c.mu, c.target,
                   c.out, c.du, c.sens ? c.sens : ws.g, c.sens != nullptr, c.status};
    hipLaunchKernelGGL(avoidance_kernel, dim3((unsigned)c.n), dim3(64), 0, st, a);
    MPCX_HIP(ctx, hipGetLastError());
    return MPCX_OK;
}

}  // namespace mpcx

using namespace mpcx;

extern "C" size_t mpcx_avoidance_workspace_bytes(int n, int S, int K)
{
    if (n < 1 || S < 1 || K < 2) return 0;
    return AvWorkspace(nullptr, n, S, K).bytes;
}

extern "C" int mpcx_avoidance_dev(mpcx_ctx *ctx, int n, const double *pairs, int S, int K, const int32_t *Ks, const double *Y, const double *U,
                                  const double *units, const double *span, const double *consts, int flags, double max_step,
                                  const double *P, int D, int cat_K, const int32_t *cat_Ks, const double *cat_Y, const double *cat_units,
                                  const double *cat_span, const double *cat_P, double mu, double target, int who, double *out, double *du,
                                  double *sens, int32_t *status, void *workspace, void *stream)
{
    if (!ctx) return MPCX_E_BADARG;
    const AvCall c = MPCX_AV_CALL;
    if (int rc = av_check(ctx, c)) return rc;
    if (!workspace) return ctx_fail(ctx, MPCX_E_BADARG, "avoidance: a workspace of mpcx_avoidance_workspace_bytes(n, S, K) bytes is required");
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    return av_enqueue(ctx, c, workspace, (hipStream_t)stream);
}

extern "C" int mpcx_avoidance(mpcx_ctx *ctx, int n, const double *pairs, int S, int K, const int32_t *Ks, const double *Y, const double *U,
                              const double *units, const double *span, const double *consts, int flags, double max_step, const double *P,
                              int D, int cat_K, const int32_t *cat_Ks, const double *cat_Y, const double *cat_units, const double *cat_span,
                              const double *cat_P, double mu, double target, int who, double *out, double *du, double *sens,
                              int32_t *status)
{
    if (!ctx) return MPCX_E_BADARG;
    const AvCall c = MPCX_AV_CALL;
    if (int rc = av_check(ctx, c)) return rc;
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    DeviceArena ar(ctx);
    AvCall d = c;
    const size_t NS = cat_Y ? 1 : 2;
    enc_upload(ar, d);
    d.out = ar.result(out, (size_t)n * MPCX_NAV);
    d.du = ar.result(du, (size_t)n * NS * 3 * K);
    d.sens = ar.result(sens, (size_t)n * NS * 9 * K);
    d.status = ar.result(status, (size_t)n);
    return host_run(ctx, ar, mpcx_avoidance_workspace_bytes(n, S, K), [&](void *ws, hipStream_t st) { return av_enqueue(ctx, d, ws, st); });
}
#undef MPCX_AV_CALL
