// covariance_drag.hip -- the covariance along trajectories with an uncertain drag (include/mpcx.h: mpcx_covariance_drag_*).
//   covariance_drag_kernel   covariance_thrust_kernel's chain over one more state: beta, the fractional error of rho C_D S / m, a
//                            first-order Gauss-Markov scalar held over each node interval.  It enters the state through the drag
//                            column G_k that the discretiser writes into the record's Sigma slot under MPCX_FLAG_DRAG_COLUMN:
//                            z = (position, velocity, mass, beta), Phi8 = [[Phi~, G~], [0, phi]], phi = exp(-h / tau_b).
// One wave per satellite, and the 8 x 8 matrices are exactly one entry per lane: lane l owns entry (l / 8, l % 8); lanes 0..20 also
// own the entries of the 7 x 3 matrices of the thrust error (C, Phi~ C, Bn~ Sigma_k, Bp~ Sigma_k+1), whose beta row is zero -- the
// thrust error is independent of beta -- and is not carried.  A node's record (its first 98 doubles) is fetched in one pass of two
// loads per lane, the next node's before the arithmetic of this one.  The operation order is fixed
// (tests/covariance_drag_reference.py restates it); LDS is ten small matrices whatever K.  The 7-term prefix of every sum over the
// state is written as covariance_thrust_kernel writes it and the beta term comes last: with sigma_b = 0 row and column 7 of P8 stay
// exact zeros, every beta term is x * 0, and P and Pm have mpcx_covariance_thrust_batch's bits, satellite by satellite in a mixed
// batch (and with a zero exec row and no mass variance mpcx_covariance_batch's).
// The status, the fills, q Q(h), the 6 x 6 block's scaling, the exec row, Sigma's column and the density row are
// covariance_device.hpp's, shared with the other two chains.  No atomics, nothing crosses a workgroup.  The linearisation is
// enc_linearise (encounter_host.hpp) with the drag column requested, once per call.
#include "collision_device.hpp"
#include "covariance_device.hpp"
#include "encounter_host.hpp"

#include <math.h>

namespace mpcx {

struct CdArgs {
    int S, K;
    const int32_t *Ks;
    const double *stage, *U, *units, *span, *P0, *q, *exec, *mvar, *dens;       // exec may be NULL: all-zero rows
    const int32_t *dstat;             // the discretiser's status [S]
    double *P, *Pm, *Pb;              // Pm, Pb may be NULL
    int32_t *status;
};

// a record's A | B_kn | B_kp | G and its room in LDS; where B_kn, B_kp and G start; the 7 x 3 matrices' entries
enum { CD_REC = 98, CD_REC_PAD = 104, CD_BN = 49, CD_BP = 70, CD_G = 91, CD_NB = 21 };

__global__ __launch_bounds__(64) void covariance_drag_kernel(CdArgs a)
{
    __shared__ double rec[CD_REC_PAD], phi[64], Pk[64], T[64];
    __shared__ double bn[CD_NB], bp[CD_NB], Ck[CD_NB], PC[CD_NB], BS[CD_NB], BT[CD_NB];
    const int s = blockIdx.x, lane = threadIdx.x;
    const bool own3 = lane < CD_NB;
    const int i = lane >> 3, j = lane & 7;
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    const bool pv = hi < 6;                                          // an entry of the position / velocity block
    const bool x7 = hi < 7;                                          // an entry of the 7 x 7 block the thrust error reaches
    const int bi = own3 ? lane / 3 : 0, bc = own3 ? lane - 3 * (lane / 3) : 0;         // entry of the 7 x 3 matrices
    const size_t K = (size_t)a.K;
    const int nn = a.Ks ? a.Ks[s] : a.K;
    const double ta = a.span[2 * s], tb = a.span[2 * s + 1], L = a.units[2 * s], Tu = a.units[2 * s + 1];
    const double qs = a.q ? a.q[s] : 0.0, mv = a.mvar ? a.mvar[s] : 0.0;
    const GatesRow ex = a.exec ? gates_load(a.exec + (size_t)s * MPCX_NEXEC) : GatesRow{0.0, 0.0, 0.0, 0.0, 0.0};
    const DensRow dn = dens_load(a.dens + (size_t)s * MPCX_NDENS);
    double pij = pv ? a.P0[(size_t)s * 36 + lo * 6 + hi] : (lane == 6 * 8 + 6 ? mv : (lane == 63 ? dn.sb * dn.sb : 0.0));      // the upper triangle alone is read
    int st = cov_status(nn, a.K, ta, tb, Tu, a.dstat + s, pv && !cp_finite(pij));
    if (st == MPCX_ST_OK && !(mv >= 0.0 && cp_finite(mv) && gates_valid(ex))) st = MPCX_ST_NUMERIC;
    if (st == MPCX_ST_OK && !dens_valid(dn)) st = MPCX_ST_NUMERIC;
    double *Ps = a.P + (size_t)s * K * 36, *Ms = a.Pm ? a.Pm + (size_t)s * K * 7 : nullptr, *Bs = a.Pb ? a.Pb + (size_t)s * K * 8 : nullptr;
    if (lane == 0) a.status[s] = st;
    if (st != MPCX_ST_OK) {
        cov_fill(Ps, lane, 0, a.K * 36, cp_nan());
        if (Ms) cov_fill(Ms, lane, 0, a.K * 7, cp_nan());
        if (Bs) cov_fill(Bs, lane, 0, a.K * 8, cp_nan());
        return;
    }
    cov_fill(Ps, lane, nn * 36, a.K * 36, 0.0);                      // columns past the satellite's count
    if (Ms) cov_fill(Ms, lane, nn * 7, a.K * 7, 0.0);
    if (Bs) cov_fill(Bs, lane, nn * 8, a.K * 8, 0.0);
    const double h = (tb - ta) / (double)(nn - 1);
    const double ph = dens_phi(dn, h);
    // the noise of one interval: q Q(h) on the 6 x 6 block, the Gauss-Markov process's (1 - phi^2) sigma_b^2 at (7, 7)
    const double qQ = lane == 63 ? (1.0 - ph * ph) * (dn.sb * dn.sb) : qs * cov_noise_entry(lo, hi, h);
    const double V = L / Tu;
    const double Di = bi < 3 ? L : (bi < 6 ? V : 1.0);               // D of the row of this lane's 7 x 3 entry
    const double Dg = i < 3 ? L : (i < 6 ? V : 1.0);                 // D of the row of this lane's 8 x 8 entry (the G~ column)
    const double *srec = a.stage + (size_t)s * (K - 1) * MPCX_STAGE_DOUBLES, *us = a.U + (size_t)s * 3 * K;
    double r0 = srec[lane], r1 = lane + 64 < CD_REC ? srec[lane + 64] : 0.0;           // the record in flight: entries lane, lane + 64 (< 98)
    double s0, s1, s2, t0 = 0.0, t1 = 0.0, t2 = 0.0;                 // column bc of Sigma_k and of Sigma_k+1
    ct_sigma_column(us, K, 0, ex, bc, s0, s1, s2);
    Pk[lane] = pij;
    if (pv) Ps[i * 6 + j] = pij;
    if (Ms && i == 6 && j < 7) Ms[j] = pij;
    if (Bs && i == 7) Bs[j] = pij;
    if (own3) Ck[lane] = 0.0;
    for (int k = 0; k + 1 < nn; ++k) {
        rec[lane] = r0;
        if (lane + 64 < CD_REC) rec[lane + 64] = r1;
        __syncthreads();
        if (k + 2 < nn) {                                            // the next node's record, ahead of this node's arithmetic
            const double *rp = srec + (size_t)(k + 1) * MPCX_STAGE_DOUBLES;
            r0 = rp[lane];
            if (lane + 64 < CD_REC) r1 = rp[lane + 64];
        }
        ct_sigma_column(us, K, k + 1, ex, bc, t0, t1, t2);
        {                                                            // Phi8 = [[D A D^-1, D G], [0, phi]], D = diag(L, L, L, V, V, V, 1)
            double v;
            if (i < 7 && j < 7) {
                const double f = rec[i * 7 + j];
                v = cov_scale6(f, i, j, Tu);
                if (j == 6 && i < 6) v = i < 3 ? f * L : f * V;
                if (i == 6 && j < 6) v = j < 3 ? f / L : f / V;
            } else if (i < 7) v = Dg * rec[CD_G + i];
            else v = j == 7 ? ph : 0.0;
            phi[lane] = v;
        }
        if (own3) { bn[lane] = Di * rec[CD_BN + lane]; bp[lane] = Di * rec[CD_BP + lane]; }
        __syncthreads();
        {                                                            // T = Phi8 P8
            double acc = phi[i * 8] * Pk[j];
#pragma unroll
            for (int m = 1; m < 7; ++m) acc = acc + phi[i * 8 + m] * Pk[m * 8 + j];
            acc = acc + phi[i * 8 + 7] * Pk[7 * 8 + j];
            T[lane] = acc;
        }
        if (own3) {                                                  // Phi~ C, Bn~ Sigma_k, Bp~ Sigma_k+1
            double pc = phi[bi * 8] * Ck[bc];
#pragma unroll
            for (int m = 1; m < 7; ++m) pc = pc + phi[bi * 8 + m] * Ck[m * 3 + bc];
            double bs = bn[bi * 3] * s0;
            bs = bs + bn[bi * 3 + 1] * s1;
            bs = bs + bn[bi * 3 + 2] * s2;
            double bt = bp[bi * 3] * t0;
            bt = bt + bp[bi * 3 + 1] * t1;
            bt = bt + bp[bi * 3 + 2] * t2;
            PC[lane] = pc; BS[lane] = bs; BT[lane] = bt;
        }
        __syncthreads();
        {                                                            // entry (lo, hi) of the new P8
            double acc = T[lo * 8] * phi[hi * 8];
#pragma unroll
            for (int m = 1; m < 7; ++m) acc = acc + T[lo * 8 + m] * phi[hi * 8 + m];
            acc = acc + T[lo * 8 + 7] * phi[hi * 8 + 7];
            if (x7) {
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
            }
            pij = acc + qQ;
        }
        Pk[lane] = pij;                                              // (this phase reads T and phi, not Pk)
        if (pv) Ps[(size_t)(k + 1) * 36 + i * 6 + j] = pij;
        if (Ms && i == 6 && j < 7) Ms[(size_t)(k + 1) * 7 + j] = pij;
        if (Bs && i == 7) Bs[(size_t)(k + 1) * 8 + j] = pij;
        if (own3) Ck[lane] = BT[lane];                               // C_k+1 = Bp~ Sigma_k+1
        s0 = t0; s1 = t1; s2 = t2;
        __syncthreads();
    }
}

// the argument tests of both entry points
static int cd_check(mpcx_ctx *ctx, int S, int K, int flags, double max_step)
{
    if (int rc = cov_check(ctx, "covariance_drag", S, K, flags, max_step)) return rc;
    if (!(flags & MPCX_FLAG_DRAG)) return enc_fail(ctx, "covariance_drag", "flags must contain MPCX_FLAG_DRAG (without drag there is no density to be uncertain about)");
    return MPCX_OK;
}

}  // namespace mpcx

using namespace mpcx;

extern "C" size_t mpcx_covariance_drag_workspace_bytes(int S, int K)
{
    if (S < 1 || K < 2) return 0;
    return LinOnlyWorkspace(nullptr, S, K).bytes;               // the linearisation's, nothing else
}

extern "C" int mpcx_covariance_drag_batch_dev(mpcx_ctx *ctx, int S, int K, const int32_t *Ks, const double *X, const double *U,
                                              const double *units, const double *span, const double *consts, int flags, double max_step,
                                              const double *P0, const double *q, const double *exec, const double *m_var0, const double *dens,
                                              double *P, double *Pm, double *Pb, int32_t *status, void *workspace, void *stream)
{
    if (!ctx) return MPCX_E_BADARG;
    if (int rc = cd_check(ctx, S, K, flags, max_step)) return rc;
    if (!X || !U || !units || !span || !consts || !P0 || !dens || !P || !status || !workspace)
        return ctx_fail(ctx, MPCX_E_BADARG, "covariance_drag: X, U, units, span, consts, P0, dens, P, status and workspace are required");
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const LinOnlyWorkspace ws(workspace, S, K);
    EncProblem lin{};
    lin.S = S; lin.K = K; lin.Ks = Ks; lin.Y = X; lin.U = U; lin.units = units; lin.span = span; lin.consts = consts;
    lin.flags = flags; lin.max_step = max_step;
    if (int rc = enc_linearise(ctx, lin, ws, st, true)) return rc;
    const CdArgs a{S, K, Ks, ws.stage, U, units, span, P0, q, exec, m_var0, dens, ws.dstat, P, Pm, Pb, status};
    hipLaunchKernelGGL(covariance_drag_kernel, dim3((unsigned)S), dim3(64), 0, st, a);
    MPCX_HIP(ctx, hipGetLastError());
    return MPCX_OK;
}

extern "C" int mpcx_covariance_drag_batch(mpcx_ctx *ctx, int S, int K, const int32_t *Ks, const double *X, const double *U,
                                          const double *units, const double *span, const double *consts, int flags, double max_step,
                                          const double *P0, const double *q, const double *exec, const double *m_var0, const double *dens,
                                          double *P, double *Pm, double *Pb, int32_t *status)
{
    if (!ctx) return MPCX_E_BADARG;
    if (int rc = cd_check(ctx, S, K, flags, max_step)) return rc;
    if (!X || !U || !units || !span || !consts || !P0 || !dens || !P || !status)
        return ctx_fail(ctx, MPCX_E_BADARG, "covariance_drag: X, U, units, span, consts, P0, dens, P and status are required");
    MPCX_HIP(ctx, hipSetDevice(ctx->device));
    DeviceArena ar(ctx);
    double *dX = ar.upload(X, (size_t)S * 7 * K), *dU = ar.upload(U, (size_t)S * 3 * K);
    double *du = ar.upload(units, (size_t)S * 2), *dsp = ar.upload(span, (size_t)S * 2), *dc = ar.upload(consts, (size_t)S * MPCX_NCONST);
    double *dP0 = ar.upload(P0, (size_t)S * 36), *dq = q ? ar.upload(q, S) : nullptr;
    double *dex = exec ? ar.upload(exec, (size_t)S * MPCX_NEXEC) : nullptr, *dmv = m_var0 ? ar.upload(m_var0, S) : nullptr;
    double *ddn = ar.upload(dens, (size_t)S * MPCX_NDENS);
    int32_t *dKs = Ks ? ar.upload(Ks, S) : nullptr;
    double *dP = ar.result(P, (size_t)S * K * 36), *dPm = ar.result(Pm, (size_t)S * K * 7), *dPb = ar.result(Pb, (size_t)S * K * 8);
    int32_t *dst = ar.result(status, (size_t)S);
    char *dws = ar.alloc<char>(mpcx_covariance_drag_workspace_bytes(S, K));
    return host_run(ctx, ar, 0, [&](void *, hipStream_t st) {
        return mpcx_covariance_drag_batch_dev(ctx, S, K, dKs, dX, dU, du, dsp, dc, flags, max_step, dP0, dq, dex, dmv, ddn, dP, dPm, dPb, dst, dws, st);
    });
}
