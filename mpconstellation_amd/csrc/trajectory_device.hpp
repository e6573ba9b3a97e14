// trajectory_device.hpp -- the geometry of a trajectory that every encounter kernel shares, each piece written once: device functions
// only, nothing of the host side, so that conjunction.hip takes it as collision_device.hpp does.
//   cp_nan, cp_inf, cp_finite, cp_dot   the quiet NaN, +inf, "a finite number", the 3-vector product
//   tr_tf                               the flight's tf of an object: its span in its own time unit, and whether that is one
//   tr_locate, tr_value_basis,          a time on nn uniform nodes over [ta, tb]: interval, s in it, the cubic Hermite bases of the
//   tr_slope_basis, tr_state            value and of the derivative there; position (m) and velocity (m/s) of a [7][ld] trajectory
//                                       (ephemeris_kernel, cp_state, mc_state; cw_basis takes the derivative basis)
//   tr_chord_start, tr_newton           the interior of the closest approach of two arcs inside one interval: the clamped minimum of
//                                       the chord, three clamped Newton steps on d . d' from it (cj_interval, mc_interval)
// The build contracts a multiply-add only inside one expression: the expressions below are the operation order of every caller, and
// the callers' results agree to the bit because they are these (tests/conjunction_reference.py, tests/collision_reference.py and
// tests/collision_mc_reference.py restate them).
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>

namespace mpcx {

__device__ __forceinline__ double cp_nan() { return __longlong_as_double(0x7ff8000000000000LL); }
__device__ __forceinline__ double cp_inf() { return __longlong_as_double(0x7ff0000000000000LL); }
__device__ __forceinline__ bool cp_finite(double x) { return fabs(x) < cp_inf(); }
__device__ __forceinline__ double cp_dot(const double (&a)[3], const double (&b)[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// tf of an object whose span is [ta, tb] seconds and whose time unit is Tu: the span in that unit.  False where that is not positive
// and finite -- an empty span, a time unit that is zero, negative or not finite: such an object is linearised and flown with tf = 1
// and the kernels that read the result give it MPCX_ST_BADK.
__device__ __forceinline__ bool tr_tf(double ta, double tb, double Tu, double &tf)
{
    tf = (tb - ta) / Tu;
    return tf > 0.0 && cp_finite(tf);
}

// where a time falls on nn uniform nodes over [ta, tb]: the node spacing, the interval k of 0 .. nn - 2 and s in it (a time outside
// the span lands in the first or the last interval with s outside [0, 1]: the callers' test)
struct TrNode {
    int k;
    double hn, sg;
};
__device__ __forceinline__ TrNode tr_locate(int nn, double ta, double tb, double t)
{
    const double hn = (tb - ta) / (double)(nn - 1);
    const double u = (t - ta) / hn;
    int k = (int)u;
    if (k > nn - 2) k = nn - 2;
    if (k < 0) k = 0;
    return TrNode{k, hn, u - (double)k};
}

// the cubic Hermite basis at s on (value at 0, slope at 0, value at 1, slope at 1), and its derivative
__device__ __forceinline__ void tr_value_basis(double s, double &h00, double &h10, double &h01, double &h11)
{
    const double s2 = s * s, s3 = s2 * s;
    h00 = 2.0 * s3 - 3.0 * s2 + 1.0; h10 = s3 - 2.0 * s2 + s; h01 = -2.0 * s3 + 3.0 * s2; h11 = s3 - s2;
}
__device__ __forceinline__ void tr_slope_basis(double s, double &g00, double &g10, double &g01, double &g11)
{
    const double s2 = s * s;
    g00 = 6.0 * s2 - 6.0 * s; g10 = 3.0 * s2 - 4.0 * s + 1.0; g01 = -6.0 * s2 + 6.0 * s; g11 = 3.0 * s2 - 2.0 * s;
}

// position p (m) and velocity v (m/s) at `nd` of a trajectory y [7][ld] in its object's units (L metres, V = L / Tu metres per
// second), h.. the value basis at nd.sg: the cubic Hermite in physical time on the node positions and velocities
__device__ __forceinline__ void tr_state(const double *y, size_t ld, const TrNode &nd, double h00, double h10, double h01, double h11, double L,
                                         double V, double (&p)[3], double (&v)[3])
{
    const int k = nd.k;
    const double hn = nd.hn;
    double g00, g10, g01, g11;
    tr_slope_basis(nd.sg, g00, g10, g01, g11);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double p0 = y[(size_t)c * ld + k] * L, p1 = y[(size_t)c * ld + k + 1] * L;
        const double m0 = hn * (y[(size_t)(3 + c) * ld + k] * V), m1 = hn * (y[(size_t)(3 + c) * ld + k + 1] * V);
        p[c] = h00 * p0 + h10 * m0 + h01 * p1 + h11 * m1;
        v[c] = (g00 * p0 + g10 * m0 + g01 * p1 + g11 * m1) / hn;
    }
}

// The relative position of two arcs inside one interval is the cubic Hermite of the end differences d0, d1 and the end relative
// velocities times the interval's length, a0, a1.  The start of the search for its closest approach: the minimum of the chord
// d0 + s (d1 - d0), clamped to [0, 1]; 0 for a chord of no (or no finite) length.
__device__ __forceinline__ double tr_chord_start(const double (&d0)[3], const double (&d1)[3])
{
    const double D[3] = {d1[0] - d0[0], d1[1] - d0[1], d1[2] - d0[2]};
    const double DD = cp_dot(D, D), b = cp_dot(d0, D);
    double s = 0.0;
    if (DD > 0.0 && DD < cp_inf()) {
        s = -b / DD;
        s = s < 0.0 ? 0.0 : (s > 1.0 ? 1.0 : s);
    }
    return s;
}

// Three Newton steps on d . d' from s, each clamped to [0, 1] and taken only where the second derivative of the squared distance
// is positive: returns the s it ends at, the squared distance there in qs.  (s comes by value: as a reference to the caller's
// variable the iterate cost track_kernel two spilled registers.)
__device__ __forceinline__ double tr_newton(const double (&d0)[3], const double (&d1)[3], const double (&a0)[3], const double (&a1)[3], double s,
                                            double &qs)
{
    double x[3];
    for (int it = 0; it < 4; ++it) {                              // three Newton steps, then the distance at the result
        double h00, h10, h01, h11;
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
    qs = cp_dot(x, x);
    return s;
}

}  // namespace mpcx
