// covariance_device.hpp -- what the two covariance chains (covariance_kernel in collision.hip, covariance_thrust_kernel in
// covariance_thrust.hip) share before their loops, and the Gates execution-error row that covariance_thrust_kernel and the Monte
// Carlo sampler (collision_mc.hip) read, each written once.
//   cov_status, cov_fill         a satellite's status (BADK / the discretiser's / a non-finite P0); NaN for a failed satellite, zero
//                                past its node count
//   cov_noise_entry              entry (lo, hi) of Q(h), the white acceleration noise of one node interval
//   cov_scale6                   an entry of the 6 x 6 block of D Phi D^-1: the transition in metres and m/s
//   GatesRow, gates_load,        a satellite's exec row (s_fm, s_pm, s_fp, s_pp, u_off): "finite and not negative", the variances
//   gates_valid, gates_on,       along and across a thrust of size |u|, and the rule that an engine at or below u_off has no error
//   gates_variances
// The chains keep their own loops: the 6 x 6 one is the cheaper and avoidance_window_refine runs it every pass.
#pragma once
#include "mpcx_host.hpp"
#include "trajectory_device.hpp"

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

}  // namespace mpcx
