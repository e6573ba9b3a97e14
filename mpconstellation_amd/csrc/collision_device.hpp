// collision_device.hpp -- the device functions of collision_probability_kernel (collision.hip) that avoidance_kernel (avoidance.hip)
// shares: one object of a pairs list at the pair's time -- its state from the cubic Hermite on its own nodes, its position
// covariance from the nearest node.  cp_object is the two steps in the order collision_probability_kernel has always run them.
#pragma once
#include "mpcx_host.hpp"

#include <math.h>

namespace mpcx {

__device__ __forceinline__ double cp_nan() { return __longlong_as_double(0x7ff8000000000000LL); }
__device__ __forceinline__ bool cp_finite(double x) { return fabs(x) < __longlong_as_double(0x7ff0000000000000LL); }

// one side of the list: the objects a pair's row or column index selects
struct CpSide {
    int N, K;
    const int32_t *Ks;
    const double *Y, *units, *span, *P, *radius;
};

// where a time falls on an object's nodes: object o, interval k of its nn nodes, s in it, the node spacing in seconds and the
// Hermite basis at s
struct CpNode {
    int o, k, nn;
    double sg, hn, h00, h10, h01, h11;
};

// Object `fidx` (an index as the pairs list holds it: a double) of one side at time t: position p, velocity v from the cubic Hermite
// on its own nodes (ephemeris_kernel's formulas).  Returns MPCX_ST_OK or MPCX_ST_BADK (no such object, a node count outside 2..K,
// an empty span, t outside the span); on BADK nothing is written and no memory of the object is read.
__device__ __forceinline__ int cp_state(const CpSide &sd, double fidx, double t, double (&p)[3], double (&v)[3], CpNode &nd)
{
    if (!(fidx >= 0.0 && fidx < (double)sd.N)) return MPCX_ST_BADK;
    const int o = (int)fidx;
    const int nn = sd.Ks ? sd.Ks[o] : sd.K;
    const double ta = sd.span[2 * o], tb = sd.span[2 * o + 1];
    if (nn < 2 || nn > sd.K || !(tb > ta) || !(t >= ta && t <= tb)) return MPCX_ST_BADK;
    const double hn = (tb - ta) / (double)(nn - 1);
    const double u = (t - ta) / hn;
    int k = (int)u;
    if (k > nn - 2) k = nn - 2;
    if (k < 0) k = 0;
    const double sg = u - (double)k, s2 = sg * sg, s3 = s2 * sg;
    const double h00 = 2.0 * s3 - 3.0 * s2 + 1.0, h10 = s3 - 2.0 * s2 + sg, h01 = -2.0 * s3 + 3.0 * s2, h11 = s3 - s2;
    const double g00 = 6.0 * s2 - 6.0 * sg, g10 = 3.0 * s2 - 4.0 * sg + 1.0, g01 = -6.0 * s2 + 6.0 * sg, g11 = 3.0 * s2 - 2.0 * sg;
    const double L = sd.units[2 * o], V = L / sd.units[2 * o + 1];
    const double *y = sd.Y + (size_t)o * 7 * sd.K;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double p0 = y[(size_t)c * sd.K + k] * L, p1 = y[(size_t)c * sd.K + k + 1] * L;
        const double m0 = hn * (y[(size_t)(3 + c) * sd.K + k] * V), m1 = hn * (y[(size_t)(3 + c) * sd.K + k + 1] * V);
        p[c] = h00 * p0 + h10 * m0 + h01 * p1 + h11 * m1;
        v[c] = (g00 * p0 + g10 * m0 + g01 * p1 + g11 * m1) / hn;
    }
    nd = CpNode{o, k, nn, sg, hn, h00, h10, h01, h11};
    return MPCX_ST_OK;
}

// Position covariance C = (c00, c01, c02, c11, c12, c22) of the object cp_state placed at `nd`: the covariance at the nearest node
// carried over dt by the short-arc two-body transition.
__device__ __forceinline__ void cp_covariance(const CpSide &sd, const CpNode &nd, double t, double mu, double (&C)[6])
{
    const int o = nd.o, k = nd.k;
    const double sg = nd.sg, hn = nd.hn, ta = sd.span[2 * o], L = sd.units[2 * o];
    const double *y = sd.Y + (size_t)o * 7 * sd.K;
    // the nearest node, the time from it, and the gravity gradient there
    const int kc = k + (sg >= 0.5 ? 1 : 0);
    const double dt = t - (ta + (double)kc * hn);
    double r[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) r[c] = y[(size_t)c * sd.K + kc] * L;
    const double r2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
    const double r1 = sqrt(r2), r5 = r2 * r2 * r1;
    const double ca = dt * dt / 2.0, cb = dt * dt * dt / 6.0;
    double F[3][6];                                                  // Phi_r = [ I + G dt^2/2 | dt I + G dt^3/6 ]
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const double G = mu * (3.0 * r[a] * r[b] - (a == b ? r2 : 0.0)) / r5;
            F[a][b] = (a == b ? 1.0 : 0.0) + G * ca;
            F[a][3 + b] = (a == b ? dt : 0.0) + G * cb;
        }
    }
    const double *Pk = sd.P + ((size_t)o * sd.K + kc) * 36;
    double M[3][6];                                                  // Phi_r P
#pragma unroll
    for (int m = 0; m < 6; ++m) {
        double col[6];
#pragma unroll
        for (int n = 0; n < 6; ++n) col[n] = Pk[n * 6 + m];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            double acc = F[a][0] * col[0];
#pragma unroll
            for (int n = 1; n < 6; ++n) acc = acc + F[a][n] * col[n];
            M[a][m] = acc;
        }
    }
    int e = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = a; b < 3; ++b) {
            double acc = M[a][0] * F[b][0];
#pragma unroll
            for (int m = 1; m < 6; ++m) acc = acc + M[a][m] * F[b][m];
            C[e++] = acc;
        }
    }
}

// cp_state, cp_covariance and the object's radius: what collision_probability_kernel needs of an object
__device__ __forceinline__ int cp_object(const CpSide &sd, double fidx, double t, double mu, double (&p)[3], double (&v)[3], double (&C)[6],
                                         double &radius)
{
    CpNode nd;
    const int st = cp_state(sd, fidx, t, p, v, nd);
    if (st != MPCX_ST_OK) return st;
    cp_covariance(sd, nd, t, mu, C);
    radius = sd.radius[nd.o];
    return MPCX_ST_OK;
}

}  // namespace mpcx
