// covariance_thrust.hip -- the covariance along trajectories with thrust execution errors (include/mpcx.h: mpcx_covariance_thrust_*).
//   covariance_thrust_kernel   chains ALL of a stage record's first 91 doubles -- A and the two first-order-hold input blocks B_kn, B_kp
//                              that mpcx_covariance_batch throws away -- into the 7 x 7 covariance of position, velocity and mass at
//                              every node, with a Gates-model execution error e_k on the thrust of every node: magnitude and pointing,
//                              each with a fixed and a proportional part.  e_k enters interval k - 1 through B_kp and interval k through
//                              B_kn, so the 7 x 3 cross-covariance C_k = Cov(x_k, e_k) is carried beside P_k.
// One wave per satellite.  Lane l < 49 owns entry (l / 7, l % 7) of the 7 x 7 matrices, lanes 0..20 also own the entries of the 7 x 3
// ones (C, Phi~ C, Bn~ Sigma_k, Bp~ Sigma_k+1).  A node's record is fetched in one pass of two loads per lane, the next node's before
// the arithmetic of this one.  Sigma_k is wave-uniform: every lane computes it from the node's thrust and keeps the column it needs.
// The operation order is fixed (tests/covariance_thrust_reference.py restates it); LDS is ten small matrices whatever K.  The 6-term
// prefix of every sum over the state is written as covariance_kernel (collision.hip) writes it: with an all-zero exec row and no
// mass variance every further term is an exact zero and P has mpcx_covariance_batch's bits, satellite by satellite in a mixed batch.
// The status, the fills, q Q(h), the 6 x 6 block's scaling and the exec row are covariance_device.hpp's, shared with that kernel;
// Sigma's column (ct_sigma_column) is there too, shared with covariance_drag_kernel.
// No atomics, nothing crosses a workgroup.  The linearisation is enc_linearise (encounter_host.hpp), as everywhere.
#include "collision_device.hpp"
#include "covariance_device.hpp"
#include "encounter_host.hpp"

#include <math.h>

namespace mpcx {

struct CtArgs {
    int S, K;
    const int32_t *Ks;
    const double *stage, *U, *units, *span, *P0, *q, *exec, *mvar;
    const int32_t *dstat;             // the discretiser's status [S]
    double *P, *Pm;                   // Pm may be NULL
    int32_t *status;
};

enum { CT_N = 7, CT_NN = 49, CT_NB = 21, CT_BN = 49, CT_BP = 70 };     // CT_BN, CT_BP: where B_kn and B_kp start in a record

__global__ __launch_bounds__(64) void covariance_thrust_kernel(CtArgs a)
{
    __shared__ double rec[CP_REC_PAD], phi[CT_NN], Pk[CT_NN], T[CT_NN];
    __shared__ double bn[CT_NB], bp[CT_NB], Ck[CT_NB], PC[CT_NB], BS[CT_NB], BT[CT_NB];
    const int s = blockIdx.x, lane = threadIdx.x;
    const bool own = lane < CT_NN, own3 = lane < CT_NB;
    const int i = own ? lane / 7 : 0, j = own ? lane - 7 * (lane / 7) : 0;
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    const bool pv = own && hi < 6;                                   // an entry of the position / velocity block
    const int bi = own3 ? lane / 3 : 0, bc = own3 ? lane - 3 * (lane / 3) : 0;         // entry of the 7 x 3 matrices
    const size_t K = (size_t)a.K;
    const int nn = a.Ks ? a.Ks[s] : a.K;
    const double ta = a.span[2 * s], tb = a.span[2 * s + 1], L = a.units[2 * s], Tu = a.units[2 * s + 1];
    const double qs = a.q ? a.q[s] : 0.0, mv = a.mvar ? a.mvar[s] : 0.0;
    const GatesRow ex = gates_load(a.exec + (size_t)s * MPCX_NEXEC);
    double pij = pv ? a.P0[(size_t)s * 36 + lo * 6 + hi] : (lane == CT_NN - 1 ? mv : 0.0);     // the upper triangle alone is read
    int st = cov_status(nn, a.K, ta, tb, Tu, a.dstat + s, pv && !cp_finite(pij));
    if (st == MPCX_ST_OK && !(mv >= 0.0 && cp_finite(mv) && gates_valid(ex))) st = MPCX_ST_NUMERIC;
    double *Ps = a.P + (size_t)s * K * 36, *Ms = a.Pm ? a.Pm + (size_t)s * K * 7 : nullptr;
    if (lane == 0) a.status[s] = st;
    if (st != MPCX_ST_OK) {
        cov_fill(Ps, lane, 0, a.K * 36, cp_nan());
        if (Ms) cov_fill(Ms, lane, 0, a.K * 7, cp_nan());
        return;
    }
    cov_fill(Ps, lane, nn * 36, a.K * 36, 0.0);                      // columns past the satellite's count
    if (Ms) cov_fill(Ms, lane, nn * 7, a.K * 7, 0.0);
    const double h = (tb - ta) / (double)(nn - 1);
    const double qQ = qs * cov_noise_entry(lo, hi, h);
    const double V = L / Tu;
    const double Di = bi < 3 ? L : (bi < 6 ? V : 1.0);               // D of the row of this lane's 7 x 3 entry
    const double *srec = a.stage + (size_t)s * (K - 1) * MPCX_STAGE_DOUBLES, *us = a.U + (size_t)s * 3 * K;
    double r0 = srec[lane], r1 = lane + 64 < CP_REC ? srec[lane + 64] : 0.0;           // the record in flight: entries lane, lane + 64 (< 91)
    double s0, s1, s2, t0 = 0.0, t1 = 0.0, t2 = 0.0;                 // column bc of Sigma_k and of Sigma_k+1
    ct_sigma_column(us, K, 0, ex, bc, s0, s1, s2);
    if (own) Pk[lane] = pij;
    if (pv) Ps[i * 6 + j] = pij;
    if (Ms && own && i == 6) Ms[j] = pij;
    if (own3) Ck[lane] = 0.0;
    for (int k = 0; k + 1 < nn; ++k) {
        rec[lane] = r0;
        if (lane + 64 < CP_REC) rec[lane + 64] = r1;
        __syncthreads();
        if (k + 2 < nn) {                                            // the next node's record, ahead of this node's arithmetic
            const double *rp = srec + (size_t)(k + 1) * MPCX_STAGE_DOUBLES;
            r0 = rp[lane];
            if (lane + 64 < CP_REC) r1 = rp[lane + 64];
        }
        ct_sigma_column(us, K, k + 1, ex, bc, t0, t1, t2);
        if (own) {                                                   // Phi~ = D A D^-1, D = diag(L, L, L, V, V, V, 1)
            const double f = rec[lane];
            double v = cov_scale6(f, i, j, Tu);
            if (j == 6 && i < 6) v = i < 3 ? f * L : f * V;
            if (i == 6 && j < 6) v = j < 3 ? f / L : f / V;
            phi[lane] = v;
        }
        if (own3) { bn[lane] = Di * rec[CT_BN + lane]; bp[lane] = Di * rec[CT_BP + lane]; }
        __syncthreads();
        if (own) {                                                   // T = Phi~ P
            double acc = phi[i * 7] * Pk[j];
#pragma unroll
            for (int m = 1; m < 7; ++m) acc = acc + phi[i * 7 + m] * Pk[m * 7 + j];
            T[lane] = acc;
        }
        if (own3) {                                                  // Phi~ C, Bn~ Sigma_k, Bp~ Sigma_k+1
            double pc = phi[bi * 7] * Ck[bc];
#pragma unroll
            for (int m = 1; m < 7; ++m) pc = pc + phi[bi * 7 + m] * Ck[m * 3 + bc];
            double bs = bn[bi * 3] * s0;
            bs = bs + bn[bi * 3 + 1] * s1;
            bs = bs + bn[bi * 3 + 2] * s2;
            double bt = bp[bi * 3] * t0;
            bt = bt + bp[bi * 3 + 1] * t1;
            bt = bt + bp[bi * 3 + 2] * t2;
            PC[lane] = pc; BS[lane] = bs; BT[lane] = bt;
        }
        __syncthreads();
        if (own) {                                                   // entry (lo, hi) of the new P
            double acc = T[lo * 7] * phi[hi * 7];
#pragma unroll
            for (int m = 1; m < 7; ++m) acc = acc + T[lo * 7 + m] * phi[hi * 7 + m];
            double y = PC[lo * 3] * bn[hi * 3];
            y = y + PC[lo * 3 + 1] * bn[hi * 3 + 1];
            y = y + PC[lo * 3 + 2] * bn[hi * 3 + 2];
            double yt = PC[hi * 3] * bn[lo * 3];
            yt = yt + PC[hi * 3 + 1] * bn[lo * 3 + 1];
            yt = yt + PC[hi * 3 + 2] * bn[lo * 3 + 2];
            const double cross = y + yt;
            acc = acc + cross;
            double n1 = BS[lo * 3] * bn[hi * 3];
            n1 = n1 + BS[lo * 3 + 1] * bn[hi * 3 + 1];
            n1 = n1 + BS[lo * 3 + 2] * bn[hi * 3 + 2];
            acc = acc + n1;
            double n2 = BT[lo * 3] * bp[hi * 3];
            n2 = n2 + BT[lo * 3 + 1] * bp[hi * 3 + 1];
            n2 = n2 + BT[lo * 3 + 2] * bp[hi * 3 + 2];
            acc = acc + n2;
            pij = acc + qQ;
            Pk[lane] = pij;
            if (pv) Ps[(size_t)(k + 1) * 36 + i * 6 + j] = pij;
            if (Ms && i == 6) Ms[(size_t)(k + 1) * 7 + j] = pij;
        }
        if (own3) Ck[lane] = BT[lane];                               // C_k+1 = Bp~ Sigma_k+1
        s0 = t0; s1 = t1; s2 = t2;
        __syncthreads();
    }
}

}  // namespace mpcx

using namespace mpcx;

extern "C" size_t mpcx_covariance_thrust_workspace_bytes(int S, int K)
{
    if (S < 1 || K < 2) return 0;
    return LinOnlyWorkspace(nullptr, S, K).bytes;               // the linearisation's, nothing else
}

extern "C" int mpcx_covariance_thrust_batch_dev(mpcx_ctx *ctx, int S, int K, const int32_t *Ks, const double *X, const double *U,
                                                const double *units, const double *span, const double *consts, int flags, double max_step,
                                                const double *P0, const double *q, const double *exec, const double *m_var0, double *P,
                                                double *Pm, int32_t *status, void *workspace, void *stream)
{
    if (!ctx) return MPCX_E_BADARG;
    if (int rc = cov_check(ctx, "covariance_thrust", S, K, flags, max_step)) return rc;
    if (!X || !U || !units || !span || !consts || !P0 || !exec || !P || !status || !workspace)
        return ctx_fail(ctx, MPCX_E_BADARG, "covariance_thrust: X, U, units, span, consts, P0, exec, P, status and workspace are required");
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const LinOnlyWorkspace ws(workspace, S, K);
    EncProblem lin{};
    lin.S = S; lin.K = K; lin.Ks = Ks; lin.Y = X; lin.U = U; lin.units = units; lin.span = span; lin.consts = consts;
    lin.flags = flags; lin.max_step = max_step;
    if (int rc = enc_linearise(ctx, lin, ws, st)) return rc;
    const CtArgs a{S, K, Ks, ws.stage, U, units, span, P0, q, exec, m_var0, ws.dstat, P, Pm, status};
    hipLaunchKernelGGL(covariance_thrust_kernel, dim3((unsigned)S), dim3(64), 0, st, a);
    MPCX_HIP(ctx, hipGetLastError());
    return MPCX_OK;
}

extern "C" int mpcx_covariance_thrust_batch(mpcx_ctx *ctx, int S, int K, const int32_t *Ks, const double *X, const double *U,
                                            const double *units, const double *span, const double *consts, int flags, double max_step,
                                            const double *P0, const double *q, const double *exec, const double *m_var0, double *P, double *Pm,
                                            int32_t *status)
{
    if (!ctx) return MPCX_E_BADARG;
    if (int rc = cov_check(ctx, "covariance_thrust", S, K, flags, max_step)) return rc;
    if (!X || !U || !units || !span || !consts || !P0 || !exec || !P || !status)
        return ctx_fail(ctx, MPCX_E_BADARG, "covariance_thrust: X, U, units, span, consts, P0, exec, P and status are required");
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    DeviceArena ar(ctx);
    double *dX = ar.upload(X, (size_t)S * 7 * K), *dU = ar.upload(U, (size_t)S * 3 * K);
    double *du = ar.upload(units, (size_t)S * 2), *dsp = ar.upload(span, (size_t)S * 2), *dc = ar.upload(consts, (size_t)S * MPCX_NCONST);
    double *dP0 = ar.upload(P0, (size_t)S * 36), *dq = q ? ar.upload(q, S) : nullptr;
    double *dex = ar.upload(exec, (size_t)S * MPCX_NEXEC), *dmv = m_var0 ? ar.upload(m_var0, S) : nullptr;
    int32_t *dKs = Ks ? ar.upload(Ks, S) : nullptr;
    double *dP = ar.result(P, (size_t)S * K * 36), *dPm = ar.result(Pm, (size_t)S * K * 7);
    int32_t *dst = ar.result(status, (size_t)S);
    char *dws = ar.alloc<char>(mpcx_covariance_thrust_workspace_bytes(S, K));
    return host_run(ctx, ar, 0, [&](void *, hipStream_t st) {
        return mpcx_covariance_thrust_batch_dev(ctx, S, K, dKs, dX, dU, du, dsp, dc, flags, max_step, dP0, dq, dex, dmv, dP, dPm, dst, dws, st);
    });
}
