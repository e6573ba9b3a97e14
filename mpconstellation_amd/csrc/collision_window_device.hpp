// collision_window_device.hpp -- the device functions of the kernels of collision_window.hip, beside the encounter core
// (collision_device.hpp), whose cp_state, CP_GL and butterflies they use.
//   an object at a time node       cw_covariance_add (the nearest node's 6 x 6 covariance carried over, added to the pair's sum)
//   the relative state at a node   cw_node: mean (d, w), the sphere rule's frame (cw_pole), the Cholesky factor of the position block
//                                  and what the conditional velocity needs of the other blocks (cw_factor); encounter_window.hip
//                                  calls cw_node as it stands for its d and L^-1
//   a row of the list              cw_row (its own tests: the window, the radius), cw_out, cw_out_empty, cw_store (its row of `out`)
//   the sphere                     cw_point (point (j, k) of the 512), cw_whiten, cw_rate (the entry rate), cw_ball_share (a lane's
//                                  64 points of the ball term)
//   the derivative                 cw_node_at (cw_node, and where the time falls on both objects' nodes), cw_rate_grad and
//                                  cw_ball_share_grad (the rate and the ball share with their gradients with respect to the mean),
//                                  cw_unwhiten, cw_basis (the Hermite bases of position and velocity on the bracketing node states):
//                                  collision_window_sensitivity_kernel and the window manoeuvres (avoidance_window_device.hpp)
// The expressions below are the operation order; tests/collision_window_reference.py restates them line by line, and
// tests/avoidance_window_reference.py the derivative's.
#pragma once
#include "collision_device.hpp"

namespace mpcx {

// numpy.polynomial.legendre.leggauss(8): node, weight on [-1, 1]
static __device__ const double CP_GL8[8][2] = {
    {-0x1.ebab1cb0acc66p-1, 0x1.9ea1d04ca0393p-4},
    {-0x1.97e4ab249f41ep-1, 0x1.c76fb531d2b91p-3},
    {-0x1.0d129583284b4p-1, 0x1.413c50a255611p-2},
    {-0x1.77ac94f3c7344p-3, 0x1.736360b19933fp-2},
    {0x1.77ac94f3c7344p-3, 0x1.736360b19933fp-2},
    {0x1.0d129583284b4p-1, 0x1.413c50a255611p-2},
    {0x1.97e4ab249f41ep-1, 0x1.c76fb531d2b91p-3},
    {0x1.ebab1cb0acc66p-1, 0x1.9ea1d04ca0393p-4},
};

// cos, sin of the azimuths (k + 1/2) 2 pi / 32 as numpy.cos, numpy.sin give them
static __device__ const double CP_AZ[32][2] = {
    {0x1.fd88da3d12526p-1, 0x1.917a6bc29b42cp-4},
    {0x1.e9f4156c62ddap-1, 0x1.294062ed59f05p-2},
    {0x1.c38b2f180bdb1p-1, 0x1.e2b5d3806f63bp-2},
    {0x1.8bc806b151741p-1, 0x1.44cf325091dd6p-1},
    {0x1.44cf325091dd6p-1, 0x1.8bc806b151741p-1},
    {0x1.e2b5d3806f63ep-2, 0x1.c38b2f180bdb0p-1},
    {0x1.294062ed59f05p-2, 0x1.e9f4156c62ddbp-1},
    {0x1.917a6bc29b438p-4, 0x1.fd88da3d12525p-1},
    {-0x1.917a6bc29b42fp-4, 0x1.fd88da3d12526p-1},
    {-0x1.294062ed59f02p-2, 0x1.e9f4156c62ddbp-1},
    {-0x1.e2b5d3806f63cp-2, 0x1.c38b2f180bdb1p-1},
    {-0x1.44cf325091dd5p-1, 0x1.8bc806b151742p-1},
    {-0x1.8bc806b151741p-1, 0x1.44cf325091dd6p-1},
    {-0x1.c38b2f180bdb0p-1, 0x1.e2b5d3806f63fp-2},
    {-0x1.e9f4156c62ddap-1, 0x1.294062ed59f06p-2},
    {-0x1.fd88da3d12525p-1, 0x1.917a6bc29b43cp-4},
    {-0x1.fd88da3d12526p-1, -0x1.917a6bc29b42bp-4},
    {-0x1.e9f4156c62ddbp-1, -0x1.294062ed59f01p-2},
    {-0x1.c38b2f180bdb1p-1, -0x1.e2b5d3806f63bp-2},
    {-0x1.8bc806b151742p-1, -0x1.44cf325091dd4p-1},
    {-0x1.44cf325091ddap-1, -0x1.8bc806b15173ep-1},
    {-0x1.e2b5d3806f63fp-2, -0x1.c38b2f180bdb0p-1},
    {-0x1.294062ed59f07p-2, -0x1.e9f4156c62ddap-1},
    {-0x1.917a6bc29b421p-4, -0x1.fd88da3d12526p-1},
    {0x1.917a6bc29b407p-4, -0x1.fd88da3d12526p-1},
    {0x1.294062ed59f00p-2, -0x1.e9f4156c62ddbp-1},
    {0x1.e2b5d3806f63ap-2, -0x1.c38b2f180bdb1p-1},
    {0x1.44cf325091dd7p-1, -0x1.8bc806b151740p-1},
    {0x1.8bc806b15173ep-1, -0x1.44cf325091ddap-1},
    {0x1.c38b2f180bdafp-1, -0x1.e2b5d3806f640p-2},
    {0x1.e9f4156c62ddap-1, -0x1.294062ed59f08p-2},
    {0x1.fd88da3d12526p-1, -0x1.917a6bc29b425p-4},
};

enum { CW_NMU = 16, CW_NAZ = 32 };                                   // the sphere rule: cos theta nodes (8 per hemisphere), azimuths
#define CW_AZW 0.09817477042468103                                   /* pi / 32: half a cos-theta interval times 2 pi / 32 */
#define CW_INV_SQRT_2PI 0.3989422804014327
#define CW_INV_SQRT2 0.7071067811865476
#define CW_INV_2PI_32 0.06349363593424097                            /* (2 pi)^-3/2 */

// The two-body gravity gradient G = mu (3 x x^T - |x|^2 I) / |x|^5 at the position x (m): cp_covariance's expression
__device__ __forceinline__ void cw_gradient(const double (&x)[3], double mu, double (&G)[3][3])
{
    const double r2 = x[0] * x[0] + x[1] * x[1] + x[2] * x[2];
    const double r1 = sqrt(r2), r5 = r2 * r2 * r1;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b) G[a][b] = mu * (3.0 * x[a] * x[b] - (a == b ? r2 : 0.0)) / r5;
    }
}

// The 6 x 6 covariance of the object cp_state placed at `nd`, added to Sg: the upper triangle row by row, (0,0) .. (0,5), (1,1) ..
// (5,5).  The covariance at the nearest node carried over dt by the short-arc two-body transition.  Position rows: [I + G0 dt^2/2 |
// dt I + G0 dt^3/6] with G0 the gradient at the node -- cp_covariance's expressions; first neglected term G' dt^3/6, order (n dt)^3.
// Velocity rows: the derivative of the position rows, d/dt Phi_r = int_0^dt G(s) Phi_r(s) ds, by Simpson's rule on the gradient at
// the node, at the middle and at the end of the arc (positions r + v s + a s^2/2 from the node's own velocity and two-body
// acceleration):  [ (G0 + 4 Gm + Ge) dt/6 + G0^2 dt^3/6 | I + (2 Gm + Ge) dt^2/6 ].  G dt and I + G dt^2/2 with the node's gradient
// alone would neglect G' dt^2/2 and G' dt^3/3 -- order (n dt)^2 in the velocity-position block; these neglect order (n dt)^4.
__device__ __forceinline__ void cw_covariance_add(const CpSide &sd, const CpNode &nd, double t, double mu, double (&Sg)[21])
{
    const int o = nd.o, k = nd.k;
    const double sg = nd.sg, hn = nd.hn, ta = sd.span[2 * o], L = sd.units[2 * o], V = L / sd.units[2 * o + 1];
    const double *y = sd.Y + (size_t)o * 7 * sd.K;
    const int kc = k + (sg >= 0.5 ? 1 : 0);
    const double dt = t - (ta + (double)kc * hn);
    double r[3], rv[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { r[c] = y[(size_t)c * sd.K + kc] * L; rv[c] = y[(size_t)(3 + c) * sd.K + kc] * V; }
    const double r2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
    const double r3 = r2 * sqrt(r2);
    const double ca = dt * dt / 2.0, cb = dt * dt * dt / 6.0, hd = 0.5 * dt, ch = hd * hd / 2.0;
    double rm[3], re[3];                                             // the arc's middle and end
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double ac = -mu * r[c] / r3;
        rm[c] = r[c] + rv[c] * hd + ac * ch;
        re[c] = r[c] + rv[c] * dt + ac * ca;
    }
    double G0[3][3], Gm[3][3], Ge[3][3];
    cw_gradient(r, mu, G0);
    cw_gradient(rm, mu, Gm);
    cw_gradient(re, mu, Ge);
    const double c6 = dt / 6.0, d6 = dt * dt / 6.0;
    double F[6][6];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const double G = G0[a][b];
            const double Q = G0[a][0] * G0[0][b] + G0[a][1] * G0[1][b] + G0[a][2] * G0[2][b];
            F[a][b] = (a == b ? 1.0 : 0.0) + G * ca;
            F[a][3 + b] = (a == b ? dt : 0.0) + G * cb;
            F[3 + a][b] = (G + 4.0 * Gm[a][b] + Ge[a][b]) * c6 + Q * cb;
            F[3 + a][3 + b] = (a == b ? 1.0 : 0.0) + (2.0 * Gm[a][b] + Ge[a][b]) * d6;
        }
    }
    const double *Pk = sd.P + ((size_t)o * sd.K + kc) * 36;
    int e = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        double M[6];                                                 // row a of Phi P
#pragma unroll
        for (int m = 0; m < 6; ++m) {
            double acc = F[a][0] * Pk[m];
#pragma unroll
            for (int n = 1; n < 6; ++n) acc = acc + F[a][n] * Pk[n * 6 + m];
            M[m] = acc;
        }
#pragma unroll
        for (int b = a; b < 6; ++b) {
            double acc = M[0] * F[b][0];
#pragma unroll
            for (int m = 1; m < 6; ++m) acc = acc + M[m] * F[b][m];
            Sg[e] = Sg[e] + acc;
            ++e;
        }
    }
}

// what the sphere loop needs of the relative state at one time node
struct CwNode {
    double d[3], w[3];                // the mean of the relative position and velocity
    double ew[3], e1[3], e2[3];       // the sphere rule's frame: the pole, then a right-handed pair across it
    double i00, i10, i11, i20, i21, i22;   // L^-1 of A = L L^T, the position block
    double W[3][3];                   // B L^-T: B A^-1 x = W (L^-1 x)
    double Sc[6];                     // D - W W^T = D - B A^-1 B^T: (0,0), (0,1), (0,2), (1,1), (1,2), (2,2)
    double cden;                      // (2 pi)^-3/2 / sqrt(det A)
};

// The sphere rule's frame: the pole along w -- the x axis when |w| is not positive --, e_1 from the coordinate axis on which |e_w| is
// smallest (the first of equal ones; cp_frame's rule for a zero miss) made orthogonal to e_w, e_2 = e_w x e_1.  False when |w| is not
// finite.
__device__ __forceinline__ bool cw_pole(CwNode &nd)
{
    const double (&w)[3] = nd.w;
    const double wn = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    const bool pos = wn > 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) nd.ew[c] = pos ? w[c] / wn : (c == 0 ? 1.0 : 0.0);
    int ax = 0;
    double ea = nd.ew[0];
    if (fabs(nd.ew[1]) < fabs(ea)) { ax = 1; ea = nd.ew[1]; }
    if (fabs(nd.ew[2]) < fabs(ea)) { ax = 2; ea = nd.ew[2]; }
#pragma unroll
    for (int c = 0; c < 3; ++c) nd.e1[c] = (c == ax ? 1.0 : 0.0) - ea * nd.ew[c];
    const double en = sqrt(nd.e1[0] * nd.e1[0] + nd.e1[1] * nd.e1[1] + nd.e1[2] * nd.e1[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c) nd.e1[c] = nd.e1[c] / en;
    nd.e2[0] = nd.ew[1] * nd.e1[2] - nd.ew[2] * nd.e1[1];
    nd.e2[1] = nd.ew[2] * nd.e1[0] - nd.ew[0] * nd.e1[2];
    nd.e2[2] = nd.ew[0] * nd.e1[1] - nd.ew[1] * nd.e1[0];
    return cp_finite(wn);
}

// From the summed 6 x 6 covariance [[A, B^T], [B, D]] (cw_covariance_add's layout): the closed-form Cholesky factor of A inverted, W,
// the Schur complement and the density's constant.  MPCX_ST_NUMERIC when a pivot is not positive and finite.
__device__ __forceinline__ int cw_factor(const double (&Sg)[21], CwNode &nd)
{
    const double a00 = Sg[0], a01 = Sg[1], a02 = Sg[2], a11 = Sg[6], a12 = Sg[7], a22 = Sg[11];
    bool ok = a00 > 0.0 && cp_finite(a00);
    const double l00 = sqrt(a00), l10 = a01 / l00, l20 = a02 / l00;
    const double r11 = a11 - l10 * l10;
    ok = ok && r11 > 0.0 && cp_finite(r11);
    const double l11 = sqrt(r11), l21 = (a12 - l20 * l10) / l11;
    const double r22 = a22 - l20 * l20 - l21 * l21;
    ok = ok && r22 > 0.0 && cp_finite(r22);
    const double l22 = sqrt(r22);
    const double i00 = 1.0 / l00, i11 = 1.0 / l11, i22 = 1.0 / l22;
    const double i10 = -(l10 * i00) * i11;
    const double i21 = -(l21 * i11) * i22;
    const double i20 = -(l20 * i00 + l21 * i10) * i22;
    nd.i00 = i00; nd.i10 = i10; nd.i11 = i11; nd.i20 = i20; nd.i21 = i21; nd.i22 = i22;
    // B [a][c] = cov(velocity a, position c) = Sg (c, 3 + a)
    const double B[3][3] = {{Sg[3], Sg[8], Sg[12]}, {Sg[4], Sg[9], Sg[13]}, {Sg[5], Sg[10], Sg[14]}};
    const double D[3][3] = {{Sg[15], Sg[16], Sg[17]}, {Sg[16], Sg[18], Sg[19]}, {Sg[17], Sg[19], Sg[20]}};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        nd.W[a][0] = B[a][0] * i00;
        nd.W[a][1] = B[a][0] * i10 + B[a][1] * i11;
        nd.W[a][2] = B[a][0] * i20 + B[a][1] * i21 + B[a][2] * i22;
    }
    int e = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = a; b < 3; ++b) nd.Sc[e++] = D[a][b] - (nd.W[a][0] * nd.W[b][0] + nd.W[a][1] * nd.W[b][1] + nd.W[a][2] * nd.W[b][2]);
    }
    nd.cden = CW_INV_2PI_32 * ((i00 * i11) * i22);
    return ok ? MPCX_ST_OK : MPCX_ST_NUMERIC;
}

// The pair (fi, fj) at the time tau: both objects by cp_state, their carried covariances summed as they are formed, the frame and
// the factor.  MPCX_ST_BADK from cp_state, MPCX_ST_NUMERIC from cw_factor or for a relative speed that is not finite.  na, nb: where
// tau falls on the two objects' nodes.
__device__ __forceinline__ int cw_node_at(const CpSide &row, const CpSide &col, double fi, double fj, double tau, double mu, CwNode &nd,
                                          CpNode &na, CpNode &nb)
{
    double pa[3], va[3], pb[3], vb[3];
    int st = cp_state(row, fi, tau, pa, va, na);
    if (st == MPCX_ST_OK) st = cp_state(col, fj, tau, pb, vb, nb);
    if (st != MPCX_ST_OK) return st;
    double Sg[21];
#pragma unroll
    for (int e = 0; e < 21; ++e) Sg[e] = 0.0;
    cw_covariance_add(row, na, tau, mu, Sg);
    cw_covariance_add(col, nb, tau, mu, Sg);
#pragma unroll
    for (int c = 0; c < 3; ++c) { nd.d[c] = pb[c] - pa[c]; nd.w[c] = vb[c] - va[c]; }
    const bool finite = cw_pole(nd);
    st = cw_factor(Sg, nd);
    return st == MPCX_ST_OK && !finite ? MPCX_ST_NUMERIC : st;
}
__device__ __forceinline__ int cw_node(const CpSide &row, const CpSide &col, double fi, double fj, double tau, double mu, CwNode &nd)
{
    CpNode na, nb;
    return cw_node_at(row, col, fi, fj, tau, mu, nd, na, nb);
}

// The row's own tests (wave-uniform) in the order of their statuses: both objects at t (na, nb), the half window h, the window
// clipped to both spans [ta, tb], the radius R = radius_i + radius_j.  R <= 0 passes: the row has no sphere (cw_out_empty).
__device__ __forceinline__ int cw_row(const CpSide &row, const CpSide &col, double fi, double fj, double t, double h, double &ta, double &tb,
                                      double &R, CpNode &na, CpNode &nb)
{
    double p[3], v[3];
    int st = cp_state(row, fi, t, p, v, na);
    if (st == MPCX_ST_OK) st = cp_state(col, fj, t, p, v, nb);
    if (st == MPCX_ST_OK && !(h > 0.0 && cp_finite(h))) st = MPCX_ST_BADK;
    if (st == MPCX_ST_OK) {
        ta = fmax(fmax(t - h, row.span[2 * na.o]), col.span[2 * nb.o]);
        tb = fmin(fmin(t + h, row.span[2 * na.o + 1]), col.span[2 * nb.o + 1]);
        if (!(tb > ta)) st = MPCX_ST_BADK;
        R = row.radius[na.o] + col.radius[nb.o];
        if (st == MPCX_ST_OK && !cp_finite(R)) st = MPCX_ST_NUMERIC;
    }
    return st;
}

// a row of `out`: the figure START + ENTRIES = total (finite), and the row without a sphere
__device__ __forceinline__ void cw_out(double (&o)[MPCX_NPW], double total, double start, double entries, double rmax, double tmax, double ta,
                                       double tb)
{
    o[MPCX_PW_P] = fmin(total, 1.0); o[MPCX_PW_START] = start; o[MPCX_PW_ENTRIES] = entries; o[MPCX_PW_RATE_MAX] = rmax;
    o[MPCX_PW_T_RATE_MAX] = tmax; o[MPCX_PW_TA] = ta; o[MPCX_PW_TB] = tb;
}
__device__ __forceinline__ void cw_out_empty(double (&o)[MPCX_NPW], double ta, double tb)
{
    o[MPCX_PW_P] = 0.0; o[MPCX_PW_START] = 0.0; o[MPCX_PW_ENTRIES] = 0.0; o[MPCX_PW_RATE_MAX] = 0.0;
    o[MPCX_PW_T_RATE_MAX] = ta; o[MPCX_PW_TA] = ta; o[MPCX_PW_TB] = tb;
}
// the row and its status to memory (one lane's work)
__device__ __forceinline__ void cw_store(const double (&o)[MPCX_NPW], int st, double *out, int32_t *status)
{
#pragma unroll
    for (int c = 0; c < MPCX_NPW; ++c) out[c] = o[c];
    *status = st;
}

// Point (j, k) of the sphere rule: cos theta node j of 16 (the 8 Gauss-Legendre nodes on [-1, 0], then on [0, 1]: the integrand's
// kink lies on the equator), azimuth k of 32 -> its weight and the unit vector n
__device__ __forceinline__ double cw_point(const CwNode &nd, int j, int k, double (&n)[3])
{
    const double mu = 0.5 * (CP_GL8[j & 7][0] + (j < 8 ? -1.0 : 1.0));
    const double st = sqrt((1.0 - mu) * (1.0 + mu));
    const double ca = CP_AZ[k][0], sa = CP_AZ[k][1];
#pragma unroll
    for (int c = 0; c < 3; ++c) n[c] = mu * nd.ew[c] + st * (ca * nd.e1[c] + sa * nd.e2[c]);
    return CP_GL8[j & 7][1] * CW_AZW;
}

// z = L^-1 (r n - d): |z|^2 is the Mahalanobis distance of the point r n from the mean
__device__ __forceinline__ void cw_whiten(const CwNode &nd, const double (&n)[3], double r, double &z0, double &z1, double &z2)
{
    const double x0 = r * n[0] - nd.d[0], x1 = r * n[1] - nd.d[1], x2 = r * n[2] - nd.d[2];
    z0 = nd.i00 * x0;
    z1 = nd.i10 * x0 + nd.i11 * x1;
    z2 = nd.i20 * x0 + nd.i21 * x1 + nd.i22 * x2;
}

// The rate at which probability enters the sphere of radius R at this node: R^2 times the sphere rule's sum of N_3(R n; d, A)
// E[(-n . nu)^+ | rho = R n], the conditional radial velocity N(v0, s2) with v0 = n . (w + W z), s2 = n^T Sc n; s2 <= 0: max(-v0, 0).
__device__ __forceinline__ double cw_rate(const CwNode &nd, double R)
{
    double acc = 0.0;
#pragma unroll 1
    for (int j = 0; j < CW_NMU; ++j) {
#pragma unroll 2
        for (int k = 0; k < CW_NAZ; ++k) {
            double n[3], z0, z1, z2;
            const double wq = cw_point(nd, j, k, n);
            cw_whiten(nd, n, R, z0, z1, z2);
            const double dens = exp(-0.5 * (z0 * z0 + z1 * z1 + z2 * z2));
            const double v0 = n[0] * (nd.w[0] + (nd.W[0][0] * z0 + nd.W[0][1] * z1 + nd.W[0][2] * z2))
                              + n[1] * (nd.w[1] + (nd.W[1][0] * z0 + nd.W[1][1] * z1 + nd.W[1][2] * z2))
                              + n[2] * (nd.w[2] + (nd.W[2][0] * z0 + nd.W[2][1] * z1 + nd.W[2][2] * z2));
            const double s2 = n[0] * (nd.Sc[0] * n[0] + nd.Sc[1] * n[1] + nd.Sc[2] * n[2]) + n[1] * (nd.Sc[1] * n[0] + nd.Sc[3] * n[1] + nd.Sc[4] * n[2])
                              + n[2] * (nd.Sc[2] * n[0] + nd.Sc[4] * n[1] + nd.Sc[5] * n[2]);
            double E;
            if (s2 > 0.0) {
                const double s = sqrt(s2), a = v0 / s;
                E = s * (exp(-0.5 * a * a) * CW_INV_SQRT_2PI) - v0 * (0.5 * erfc(a * CW_INV_SQRT2));
            } else {
                E = fmax(-v0, 0.0);
            }
            acc = acc + wq * (dens * E);
        }
    }
    return ((R * R) * nd.cden) * acc;
}

// Lane `lane`'s share of the ball term P(|rho| <= R) at this node: radius node lane / 8 of the 8 Gauss-Legendre radii on [0, R], the
// cos theta nodes 2 (lane % 8) and 2 (lane % 8) + 1 with all azimuths.  The wave's sum times cden is the probability.
__device__ __forceinline__ double cw_ball_share(const CwNode &nd, double R, int lane)
{
    const int i = lane >> 3, j0 = 2 * (lane & 7);
    const double r = R * (0.5 + 0.5 * CP_GL8[i][0]);
    const double wr = ((0.5 * R) * CP_GL8[i][1]) * (r * r);
    double acc = 0.0;
#pragma unroll 1
    for (int j = j0; j < j0 + 2; ++j) {
#pragma unroll 2
        for (int k = 0; k < CW_NAZ; ++k) {
            double n[3], z0, z1, z2;
            const double wq = cw_point(nd, j, k, n);
            cw_whiten(nd, n, r, z0, z1, z2);
            acc = acc + wq * exp(-0.5 * (z0 * z0 + z1 * z1 + z2 * z2));
        }
    }
    return wr * acc;
}

// ---- the derivative with respect to the mean relative state (collision_window_sensitivity_kernel, avoidance_window_kernel)

// L^-T u
__device__ __forceinline__ void cw_unwhiten(const CwNode &nd, double u0, double u1, double u2, double (&x)[3])
{
    x[0] = nd.i00 * u0 + nd.i10 * u1 + nd.i20 * u2;
    x[1] = nd.i11 * u1 + nd.i21 * u2;
    x[2] = nd.i22 * u2;
}

// cw_rate and its derivative with respect to the mean (d, w) at fixed covariance and frame -> the rate (cw_rate's bits: the same
// expressions), cg = (d rate / d d | d rate / d w).  Per point, with Phi = Phi(-v0 / s) (s2 <= 0: 1 where v0 < 0, else 0):
//   d/dd [N_3 E] = N_3 L^-T (E z + Phi W^T n),   d/dw [N_3 E] = -N_3 Phi n;
// the whitened sums u = sum wq dens (E z + Phi W^T n) and v = sum wq dens Phi n run with the rate's, L^-T is applied once.
__device__ __forceinline__ double cw_rate_grad(const CwNode &nd, double R, double (&cg)[6])
{
    double acc = 0.0, u0 = 0.0, u1 = 0.0, u2 = 0.0, v0s = 0.0, v1s = 0.0, v2s = 0.0;
#pragma unroll 1
    for (int j = 0; j < CW_NMU; ++j) {
#pragma unroll 1
        for (int k = 0; k < CW_NAZ; ++k) {
            double n[3], z0, z1, z2;
            const double wq = cw_point(nd, j, k, n);
            cw_whiten(nd, n, R, z0, z1, z2);
            const double dens = exp(-0.5 * (z0 * z0 + z1 * z1 + z2 * z2));
            const double v0 = n[0] * (nd.w[0] + (nd.W[0][0] * z0 + nd.W[0][1] * z1 + nd.W[0][2] * z2))
                              + n[1] * (nd.w[1] + (nd.W[1][0] * z0 + nd.W[1][1] * z1 + nd.W[1][2] * z2))
                              + n[2] * (nd.w[2] + (nd.W[2][0] * z0 + nd.W[2][1] * z1 + nd.W[2][2] * z2));
            const double s2 = n[0] * (nd.Sc[0] * n[0] + nd.Sc[1] * n[1] + nd.Sc[2] * n[2]) + n[1] * (nd.Sc[1] * n[0] + nd.Sc[3] * n[1] + nd.Sc[4] * n[2])
                              + n[2] * (nd.Sc[2] * n[0] + nd.Sc[4] * n[1] + nd.Sc[5] * n[2]);
            double E, Phi;
            if (s2 > 0.0) {
                const double s = sqrt(s2), a = v0 / s;
                Phi = 0.5 * erfc(a * CW_INV_SQRT2);
                E = s * (exp(-0.5 * a * a) * CW_INV_SQRT_2PI) - v0 * Phi;
            } else {
                Phi = v0 < 0.0 ? 1.0 : 0.0;
                E = fmax(-v0, 0.0);
            }
            acc = acc + wq * (dens * E);
            const double wd = wq * dens, wp = wd * Phi;
            u0 = u0 + wd * (E * z0 + Phi * (nd.W[0][0] * n[0] + nd.W[1][0] * n[1] + nd.W[2][0] * n[2]));
            u1 = u1 + wd * (E * z1 + Phi * (nd.W[0][1] * n[0] + nd.W[1][1] * n[1] + nd.W[2][1] * n[2]));
            u2 = u2 + wd * (E * z2 + Phi * (nd.W[0][2] * n[0] + nd.W[1][2] * n[1] + nd.W[2][2] * n[2]));
            v0s = v0s + wp * n[0]; v1s = v1s + wp * n[1]; v2s = v2s + wp * n[2];
        }
    }
    const double sc = (R * R) * nd.cden;
    double gd[3];
    cw_unwhiten(nd, u0, u1, u2, gd);
    cg[0] = sc * gd[0]; cg[1] = sc * gd[1]; cg[2] = sc * gd[2];
    cg[3] = -(sc * v0s); cg[4] = -(sc * v1s); cg[5] = -(sc * v2s);
    return sc * acc;
}

// cw_ball_share (its bits) and the lane's share gz of the whitened sum of N_3 z over the ball: cden L^-T (the wave's sum of gz) is
// the derivative of the ball term with respect to d
__device__ __forceinline__ double cw_ball_share_grad(const CwNode &nd, double R, int lane, double (&gz)[3])
{
    const int i = lane >> 3, j0 = 2 * (lane & 7);
    const double r = R * (0.5 + 0.5 * CP_GL8[i][0]);
    const double wr = ((0.5 * R) * CP_GL8[i][1]) * (r * r);
    double acc = 0.0, a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll 1
    for (int j = j0; j < j0 + 2; ++j) {
#pragma unroll 2
        for (int k = 0; k < CW_NAZ; ++k) {
            double n[3], z0, z1, z2;
            const double wq = cw_point(nd, j, k, n);
            cw_whiten(nd, n, r, z0, z1, z2);
            const double ex = exp(-0.5 * (z0 * z0 + z1 * z1 + z2 * z2));
            acc = acc + wq * ex;                                         // (cw_ball_share's expression: one multiply-add)
            const double e = wq * ex;
            a0 = a0 + e * z0; a1 = a1 + e * z1; a2 = a2 + e * z2;
        }
    }
    gz[0] = wr * a0; gz[1] = wr * a1; gz[2] = wr * a2;
    return wr * acc;
}

// How the position (m) and the velocity (m/s) of an object at a time inside interval k of its nodes depend on the two bracketing node
// states in normalised units, (y_pos[k], y_vel[k], y_pos[k+1], y_vel[k+1]): cp_state's Hermite bases h.. and g.., the position's in
// mpcx_avoidance's form L [h I | h_tau h I]
struct CwBasis {
    double p[4], v[4];
};
__device__ __forceinline__ void cw_basis(const CpNode &nd, double L, double Tu, double htau, CwBasis &b)
{
    double g00, g10, g01, g11;
    tr_slope_basis(nd.sg, g00, g10, g01, g11);
    const double V = L / Tu;
    b.p[0] = L * nd.h00; b.p[1] = L * (htau * nd.h10); b.p[2] = L * nd.h01; b.p[3] = L * (htau * nd.h11);
    b.v[0] = (L * g00) / nd.hn; b.v[1] = V * g10; b.v[2] = (L * g01) / nd.hn; b.v[3] = V * g11;
}

}  // namespace mpcx
