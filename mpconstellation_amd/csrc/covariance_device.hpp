// covariance_device.hpp -- what the three covariance chains (covariance_kernel in collision.hip, covariance_thrust_kernel in
// covariance_thrust.hip, covariance_drag_kernel in covariance_drag.hip) share before their loops, the Gates execution-error row that
// the last two and the Monte Carlo sampler (collision_mc.hip) read, and the density row of the third, each written once.
//   cov_status, cov_fill         a satellite's status (BADK / the discretiser's / a non-finite P0); NaN for a failed satellite, zero
//                                past its node count
//   cov_noise_entry              entry (lo, hi) of Q(h), the white acceleration noise of one node interval
//   cov_scale6                   an entry of the 6 x 6 block of D Phi D^-1: the transition in metres and m/s
//   GatesRow, gates_load,        a satellite's exec row (s_fm, s_pm, s_fp, s_pp, u_off): "finite and not negative", the variances
//   gates_valid, gates_on,       along and across a thrust of size |u|, and the rule that an engine at or below u_off has no error
//   gates_variances
//   ct_sigma_column              a column of the execution-error covariance Sigma_k of a node of a thrust table
//   DensRow, dens_load,          a satellite's density row (sigma_b, tau_b), its validity and the interval's phi = exp(-h / tau_b)
//   dens_valid, dens_phi
// The chains keep their own loops: the 6 x 6 one is the cheaper and avoidance_window_refine runs it every pass.
#pragma once
#include "mpcx_host.hpp"
#include "trajectory_device.hpp"

#include <math.h>

namespace mpcx {

// The status of satellite s of a chain, wave-uniform: MPCX_ST_BADK for a node count outside 2 .. K, an empty span or no positive
// finite tf (tr_tf: the linearisation ran with tf = 1), else the discretiser's, else MPCX_ST_NUMERIC where a lane holds an entry of P0
// that is not finite.  Called by the whole wave.
__device__ __forceinline__ int cov_status(int nn, int K, double ta, double tb, double Tu, const int32_t *dstat, bool p0_bad)
{
    double tfv;
    if (nn < 2 || nn > K || !(tb > ta) || !tr_tf(ta, tb, Tu, tfv)) return MPCX_ST_BADK;
    if (*dstat != MPCX_ST_OK) return *dstat;
    if (__any(p0_bad)) return MPCX_ST_NUMERIC;
    return MPCX_ST_OK;
}

// x[from .. to) = v by the 64 lanes of the wave: NaN throughout for a failed satellite, zero in the columns past its count
__device__ __forceinline__ void cov_fill(double *x, int lane, int from, int to, double v)
{
    for (int e = from + lane; e < to; e += 64) x[e] = v;
}

// Q(h), entry (lo <= hi): [[h^3/3 I, h^2/2 I], [h^2/2 I, h I]] on the position / velocity block, nothing on the mass
__device__ __forceinline__ double cov_noise_entry(int lo, int hi, double h)
{
    double Qe = 0.0;
    if (hi < 3) Qe = lo == hi ? h * h * h / 3.0 : 0.0;
    else if (lo < 3) Qe = hi - 3 == lo ? h * h / 2.0 : 0.0;
    else if (hi < 6) Qe = lo == hi ? h : 0.0;
    return Qe;
}

// entry (i, j < 6) of D Phi D^-1 from the entry f of Phi in the satellite's units, D = diag(L, L, L, V, V, V): the length unit cancels
__device__ __forceinline__ double cov_scale6(double f, int i, int j, double Tu)
{
    return i < 3 && j >= 3 ? f * Tu : (i >= 3 && j < 3 ? f / Tu : f);
}

// a satellite's exec row in its own thrust unit
struct GatesRow {
    double fm, pm, fp, pp, off;
};
__device__ __forceinline__ GatesRow gates_load(const double *row) { return GatesRow{row[0], row[1], row[2], row[3], row[4]}; }

__device__ __forceinline__ bool gates_valid(const GatesRow &ex)
{
    return ex.fm >= 0.0 && cp_finite(ex.fm) && ex.pm >= 0.0 && cp_finite(ex.pm) && ex.fp >= 0.0 && cp_finite(ex.fp) && ex.pp >= 0.0 &&
           cp_finite(ex.pp) && ex.off >= 0.0 && cp_finite(ex.off);
}

// the engine is on at a node whose thrust has size un (a size that is not a number counts as off)
__device__ __forceinline__ bool gates_on(const GatesRow &ex, double un) { return un > ex.off; }

// the variances of the execution error along (par) and across (perp) a thrust of size un
__device__ __forceinline__ void gates_variances(const GatesRow &ex, double un, double &par, double &perp)
{
    const double a = ex.pm * un, b = ex.pp * un;
    par = ex.fm * ex.fm + a * a; perp = ex.fp * ex.fp + b * b;
}

// Column c of Sigma of node k of the thrust table u (rows K apart).  Zero when the engine is off (|u| <= u_off; a |u| that is not a
// number counts as off).  Wave-uniform but for the choice of the column.
__device__ __forceinline__ void ct_sigma_column(const double *u, size_t K, int k, const GatesRow &ex, int c, double &c0, double &c1, double &c2)
{
    const double ux = u[k], uy = u[K + k], uz = u[2 * K + k];
    const double un = sqrt(ux * ux + uy * uy + uz * uz);
    c0 = 0.0; c1 = 0.0; c2 = 0.0;
    if (!gates_on(ex, un)) return;
    const double hx = ux / un, hy = uy / un, hz = uz / un;
    double sp, sq;
    gates_variances(ex, un, sp, sq);
    const double xx = hx * hx, xy = hx * hy, xz = hx * hz, yy = hy * hy, yz = hy * hz, zz = hz * hz;
    const double sxx = sp * xx + sq * (1.0 - xx), sxy = sp * xy - sq * xy, sxz = sp * xz - sq * xz;
    const double syy = sp * yy + sq * (1.0 - yy), syz = sp * yz - sq * yz;
    const double szz = sp * zz + sq * (1.0 - zz);
    c0 = c == 0 ? sxx : (c == 1 ? sxy : sxz);
    c1 = c == 0 ? sxy : (c == 1 ? syy : syz);
    c2 = c == 0 ? sxz : (c == 1 ? syz : szz);
}

// A satellite's density row (sigma_b, tau_b) of mpcx_covariance_drag_batch: beta, the fractional error of rho C_D S / m, is a first-order
// Gauss-Markov process with stationary deviation sigma_b and correlation time tau_b in seconds (+inf: a constant bias), held over
// each node interval.  Valid: sigma_b finite and not negative, tau_b > 0 (a NaN is not).
struct DensRow {
    double sb, tau;
};
__device__ __forceinline__ DensRow dens_load(const double *row) { return DensRow{row[0], row[1]}; }
__device__ __forceinline__ bool dens_valid(const DensRow &d) { return d.sb >= 0.0 && cp_finite(d.sb) && d.tau > 0.0; }
// phi = exp(-h / tau_b) over a node spacing of h seconds: exactly 1 for tau_b = +inf
__device__ __forceinline__ double dens_phi(const DensRow &d, double h) { return exp(-h / d.tau); }

}  // namespace mpcx
