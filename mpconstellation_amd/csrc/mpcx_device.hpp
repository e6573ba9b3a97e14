// mpcx_device.hpp -- device-side building blocks shared by the gfx950 kernels.
// fp64 throughout.  Written for CDNA4 (wave64); no other target is supported.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mpcx.h"
#include "integrator_device.hpp"

namespace mpcx {

constexpr double kCd = 2.5;             // constants.py:7
constexpr double kRho500 = 9.983E-13;   // simulator.py:112
constexpr double kEps = 2.220446049250313e-16;
constexpr double kREarth = 6.371E6;     // constants.py:3 (metres)

// Python / numpy float floor division (the `tau // dtau` of linearize_discretize.py:310)
__device__ __forceinline__ double py_floordiv(double a, double b)
{
    double mod = fmod(a, b);
    double div = (a - mod) / b;
    if (mod != 0.0 && ((b < 0) != (mod < 0))) div -= 1.0;
    if (div != 0.0) {
        double fl = floor(div);
        if (div - fl > 0.5) fl += 1.0;
        return fl;
    }
    return copysign(0.0, a / b);
}

// 1/d and 1/sqrt(d) for d > 0 well inside the normal range: hardware seed + two Newton steps instead of the IEEE division /
// square-root sequences (scaling, fix-up: ~3x the instructions), which pivots, slacks, determinants and the norms of the
// right-hand sides do not need.  Measured on gfx950 over 1e-40..1e40 (profiles/tools/rcp_accuracy.hip): seed 4.5e-8 relative,
// one step 2.1e-15, two steps 1.1e-16 = half an ulp.
__device__ __forceinline__ double rcp_pos(double d)
{
    double r = __builtin_amdgcn_rcp(d);
#pragma unroll
    for (int n = 0; n < 2; ++n) { const double e = fma(-d, r, 1.0); r = fma(r, e, r); }
    return r;
}
__device__ __forceinline__ double rsq_pos(double d)
{
    double r = __builtin_amdgcn_rsq(d);
#pragma unroll
    for (int n = 0; n < 2; ++n) { const double e = fma(-d * r, r, 1.0); r = fma(0.5 * r, e, r); }
    return r;
}

// The node of a first-order hold over Ku columns at tau != 1 (linearize_discretize.py:305-312, control.py:104-126):
// k = int(tau // dtau), dtau = 1 / (Ku - 1); the hold interpolates columns k and k + 1.  Where the reference raises IndexError
// (k < 0 or k + 1 >= Ku) err becomes MPCX_ST_FOH and k the nearest interval's; a table without an interval (Ku < 2) then
// returns false: the hold is zero.  (tau == 1, the last column itself, is the caller's line before this: with it in here the
// three holds' kernels are allocated other registers)
// QUICK: floor(tau (Ku - 1)) is the floor of the exact quotient (Python's float floor division goes through an exact fmod) unless
// the product sits within rounding of an integer, and only then the exact routine is called.
template <bool QUICK = false>
__device__ __forceinline__ bool foh_node(double tau, int Ku, int &k, int &err)
{
    const double km1 = (double)(Ku - 1);
    if constexpr (QUICK) {
        const double q = tau * km1;
        k = (fabs(q - rint(q)) > 1e-9 * fmax(1.0, q)) ? (int)floor(q) : (int)py_floordiv(tau, 1.0 / km1);
    } else k = (int)py_floordiv(tau, 1.0 / km1);
    if (k < 0 || k + 1 >= Ku) {
        err = MPCX_ST_FOH;
        k = k < 0 ? 0 : Ku - 2;
        if (Ku < 2) return false;
    }
    return true;
}

// First-order hold of a (3,Ku) row-major table: linearize_discretize.py:294-315, control.py:104-126
// (ld: row length of the table in memory, Ku <= ld of its columns in use -- they differ only in ragged batches)
__device__ __forceinline__ void foh3(double tau, const double *__restrict__ u, int Ku, int ld, double (&out)[3],
                                     int &err)
{
    if (tau == 1.0) {
        out[0] = u[Ku - 1]; out[1] = u[ld + Ku - 1]; out[2] = u[2 * ld + Ku - 1];
        return;
    }
    int k;
    if (!foh_node(tau, Ku, k, err)) { out[0] = out[1] = out[2] = 0.0; return; }
    const double km1 = (double)(Ku - 1);
    const double tau_k = (double)k / km1, tau_kp1 = (double)(k + 1) / km1;
    const double lam_n = (tau_kp1 - tau) / (tau_kp1 - tau_k);
    const double lam_p = (tau - tau_k) / (tau_kp1 - tau_k);
    out[0] = lam_n * u[k] + lam_p * u[k + 1];
    out[1] = lam_n * u[ld + k] + lam_p * u[ld + k + 1];
    out[2] = lam_n * u[2 * ld + k] + lam_p * u[2 * ld + k + 1];
}

// The same first-order hold with the interval in use kept in registers: the two table columns, the node index and the
// interval's end points are reloaded / recomputed only when tau leaves the cached interval (an RK45 step is short
// against 1/(Ku-1): the stages of a step and many steps in a row stay inside one interval).  Inside -- away from both
// ends by more than any rounding of the index computation -- k is certain and the weights are foh3's up to one rounding
// (multiplication by the interval's cached reciprocal length instead of two divisions); otherwise -- node times included --
// foh3's own index computation and expressions decide.  Saves the fmod of py_floordiv, two divisions and six dependent
// global loads per right-hand side.
struct FohCache {
    int k;
    double tau_k, tau_kp1, inv, uk[3], uk1[3];
    __device__ __forceinline__ void reset() { k = -1; tau_k = 2.0; tau_kp1 = -1.0; inv = 0.0; }
};

__device__ __forceinline__ void foh3_cached(double tau, const double *__restrict__ u, int Ku, int ld, FohCache &c, double (&out)[3],
                                            int &err)
{
    if (!(tau > c.tau_k + 1e-12 && tau < c.tau_kp1 - 1e-12)) {      // rare: everything but "same interval" is behind this branch
        if (tau == 1.0) {
            out[0] = u[Ku - 1]; out[1] = u[ld + Ku - 1]; out[2] = u[2 * ld + Ku - 1];
            return;
        }
        int k;
        if (!foh_node(tau, Ku, k, err)) { out[0] = out[1] = out[2] = 0.0; return; }
        if (k != c.k) {
            const double km1 = (double)(Ku - 1);
            c.k = k;
            c.tau_k = (double)k / km1; c.tau_kp1 = (double)(k + 1) / km1;
#pragma unroll
            for (int i = 0; i < 3; ++i) { c.uk[i] = u[i * ld + k]; c.uk1[i] = u[i * ld + k + 1]; }
            c.inv = 1.0 / (c.tau_kp1 - c.tau_k);
        }
        const double lam_n = (c.tau_kp1 - tau) / (c.tau_kp1 - c.tau_k);
        const double lam_p = (tau - c.tau_k) / (c.tau_kp1 - c.tau_k);
#pragma unroll
        for (int i = 0; i < 3; ++i) out[i] = lam_n * c.uk[i] + lam_p * c.uk1[i];
        return;
    }
    const double lam_n = (c.tau_kp1 - tau) * c.inv, lam_p = (tau - c.tau_k) * c.inv;
#pragma unroll
    for (int i = 0; i < 3; ++i) out[i] = lam_n * c.uk[i] + lam_p * c.uk1[i];
}

// bcast8 for a 32-bit integer
template <int Q>
__device__ __forceinline__ int bcast8i(int v)
{
    const int t = __builtin_amdgcn_update_dpp(0, v, 0x150 + Q, 0xF, 0xF, true);
    return __builtin_amdgcn_update_dpp(t, v, 0x150 + 8 + Q, 0xF, 0xC, false);
}

// Value of lane q of the caller's 8-lane group in all 8 lanes (q a compile-time constant): two v_mov_b64_dpp -- gfx950 has
// the 64-bit DPP move for row_newbcast -- lane q of every 16-lane row into the whole row, then lane 8 + q over the row's
// upper half under a bank mask.  VALU only: no ds_bpermute, no LDS round trip.  Checked against __shfl for every q by
// profiles/tools/dpp_bcast_check.hip.
template <int Q>
__device__ __forceinline__ double bcast8(double v)
{
    const long long b = __double_as_longlong(v);
    const long long t = __builtin_amdgcn_update_dpp((long long)0, b, 0x150 + Q, 0xF, 0xF, true);
    return __longlong_as_double(__builtin_amdgcn_update_dpp(t, b, 0x150 + 8 + Q, 0xF, 0xC, false));
}

// Sum over the caller's 8-lane group, bitwise identical on its 8 lanes: neighbours inside the quad by quad_perm, then the
// other quad by row_half_mirror (lane i <-> 7 - i; both quads hold their quad's sum by then and a + b = b + a bit for bit).
template <int CTRL>
__device__ __forceinline__ double dpp64(double v)
{
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)b, CTRL, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xF, 0xF, true);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
__device__ __forceinline__ double group_sum8(double v)
{
    v += dpp64<0xB1>(v);      // quad_perm [1,0,3,2]
    v += dpp64<0x4E>(v);      // quad_perm [2,3,0,1]
    v += dpp64<0x141>(v);     // row_half_mirror
    return v;
}

struct SatConst {
    double mu, re, j2, g0, isp, s, r0, rho;
    __device__ __forceinline__ void load(const double *__restrict__ c)
    {
        mu = c[MPCX_C_MU]; re = c[MPCX_C_R_E]; j2 = c[MPCX_C_J2]; g0 = c[MPCX_C_G0];
        isp = c[MPCX_C_ISP]; s = c[MPCX_C_S]; r0 = c[MPCX_C_R0]; rho = c[MPCX_C_RHO];
    }
};

// The altitude-dependent atmosphere (MPCX_FLAG_ATMO, include/mpcx.h: atm = {c0, c1, c2, h_floor}, physical units):
//   h = max(|r R0| - R_EARTH, h_floor) metres (the altitude of simulator.py:109),  rho(h) = exp(c0 + c1 ln h + c2 h) kg/m^3.
// d2 = |r R0|^2, the sum of the squared components r_i R0 (the rollout's lanes hold one component each and bring the quad's
// sum).  Returns rho / c.rho, what the drag acceleration multiplies where the fixed model has kRho500 / c.rho; with drho given,
// also d(rho / c.rho) / d|r| = rho (c1 / h + c2) R0 / c.rho above the floor and 0 on it -- the reference's drho_func
// (linearize_discretize.py:165-166).  A trial stage that lands below the floor (or at a NaN) is evaluated on the floor.
__device__ __forceinline__ double atmo_density(double d2, const SatConst &c, const double (&atm)[MPCX_NATMO], double *drho = nullptr)
{
    const double alt = sqrt(d2) - kREarth;
    const bool above = alt > atm[MPCX_ATMO_HFLOOR];
    const double h = above ? alt : atm[MPCX_ATMO_HFLOOR];
    const double rho = exp(atm[MPCX_ATMO_C0] + atm[MPCX_ATMO_C1] * log(h) + atm[MPCX_ATMO_C2] * h) / c.rho;
    if (drho) *drho = above ? rho * (atm[MPCX_ATMO_C1] / h + atm[MPCX_ATMO_C2]) * c.r0 : 0.0;
    return rho;
}
__device__ __forceinline__ double atmo_density(const double (&r)[3], const SatConst &c, const double (&atm)[MPCX_NATMO], double *drho = nullptr)
{
    const double p[3] = {r[0] * c.r0, r[1] * c.r0, r[2] * c.r0};
    return atmo_density(p[0] * p[0] + p[1] * p[1] + p[2] * p[2], c, atm, drho);
}

// The scalar rules of Simulator.satellite_dynamics' perturbations (simulator.py:150-158; oracle/dynamics.c has the plain form), as the
// rollout's right-hand side and the discretiser's linearisation both apply them (im = 1 / m):
//   drag:  a_D = drag_k (rho / c.rho) |v| v,  drag_k = -C_D S / (2 m); fixed_density: rho / c.rho of the fixed model (atmo_density
//          otherwise);
//   J2:    a_J2,i = j2_factor / |r|^5 (5 q^2 - {1, 1, 3}_i) r_i,  q = r_z / |r|.
__device__ __forceinline__ double drag_k(const SatConst &c, double im) { return -0.5 * kCd * c.s * im; }
__device__ __forceinline__ double fixed_density(const SatConst &c) { return kRho500 / c.rho; }
__device__ __forceinline__ double j2_factor(const SatConst &c) { return 1.5 * c.j2 * c.mu * (c.re * c.re); }
__device__ __forceinline__ double j2_bracket(double q2, int comp) { return 5.0 * q2 - (comp == 2 ? 3.0 : 1.0); }

}  // namespace mpcx
