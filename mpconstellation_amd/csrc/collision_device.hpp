// collision_device.hpp -- the encounter core: the device functions that collision_probability_kernel (collision.hip), avoidance_kernel
// (avoidance.hip) and aj_rows_kernel / aj_solve_kernel / ar_trhs_kernel (avoidance_joint.hip) share, each written once.
//   (trajectory_device.hpp)        cp_nan, cp_inf, cp_finite, cp_dot, tr_tf and the cubic Hermite of a trajectory, below everything here
//   an object at the pair's time   cp_state (tr_state on its own nodes, behind the object's tests), cp_covariance (the nearest node's covariance carried
//                                  over), cp_object (both, in the order collision_probability_kernel has always run them)
//   the encounter                  cp_frame (e_1, e_2, e_w, the miss and the speed), cp_plane_covariance (C_2 = E^T Cs E, its eigenvalues)
//   the thrust sensitivities       cp_mover (what a manoeuvring object brings to the sweep), cp_sweep_seed, cp_sweep_node (one node of
//                                  the adjoint recursion, g_m stored), aj_sweep (the recursion for NR rows on a whole wave)
//   cp_wave_sum, cp_wave_max       the xor butterfly: every lane ends with the same bits
//   CP_GL                          the 64-point Gauss-Legendre rule, one copy for collision_probability_kernel and
//                                  collision_window_kernel (collision_window.hip; its own functions: collision_window_device.hpp)
// The build contracts a multiply-add only inside one expression: the expressions below are the operation order of all three files
// (tests/collision_reference.py and tests/avoidance_reference.py restate them).
#pragma once
#include "mpcx_host.hpp"
#include "trajectory_device.hpp"

#include <math.h>

namespace mpcx {

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
// on its own nodes (tr_state, as ephemeris_kernel).  Returns MPCX_ST_OK or MPCX_ST_BADK (no such object, a node count outside 2..K,
// an empty span, t outside the span); on BADK nothing is written and no memory of the object is read.
__device__ __forceinline__ int cp_state(const CpSide &sd, double fidx, double t, double (&p)[3], double (&v)[3], CpNode &nd)
{
    if (!(fidx >= 0.0 && fidx < (double)sd.N)) return MPCX_ST_BADK;
    const int o = (int)fidx;
    const int nn = sd.Ks ? sd.Ks[o] : sd.K;
    const double ta = sd.span[2 * o], tb = sd.span[2 * o + 1];
    if (nn < 2 || nn > sd.K || !(tb > ta) || !(t >= ta && t <= tb)) return MPCX_ST_BADK;
    const TrNode at = tr_locate(nn, ta, tb, t);
    double h00, h10, h01, h11;
    tr_value_basis(at.sg, h00, h10, h01, h11);
    const double L = sd.units[2 * o], V = L / sd.units[2 * o + 1];
    tr_state(sd.Y + (size_t)o * 7 * sd.K, (size_t)sd.K, at, h00, h10, h01, h11, L, V, p, v);
    nd = CpNode{o, at.k, nn, at.sg, at.hn, h00, h10, h01, h11};
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

// numpy.polynomial.legendre.leggauss(64): node, weight on [-1, 1] (collision_probability_kernel; the time rule of
// collision_window_kernel)
static __device__ const double CP_GL[64][2] = {
    {-0x1.ffa4e911f7533p-1, 0x1.d379f1845dc3ap-10},
    {-0x1.fe204ab274eccp-1, 0x1.0fc7ac3ac343cp-8},
    {-0x1.fb661ac8c85a9p-1, 0x1.aa46b24145fd3p-8},
    {-0x1.f777d976cfadap-1, 0x1.21e400109d579p-7},
    {-0x1.f257e4db5aabcp-1, 0x1.6df524de84ee7p-7},
    {-0x1.ec09586b58faap-1, 0x1.b9283b35df9afp-7},
    {-0x1.e490081f2891bp-1, 0x1.01a7c0a5c98e8p-6},
    {-0x1.dbf07d935a5afp-1, 0x1.261ef40a7a2dbp-6},
    {-0x1.d22ff5221288ap-1, 0x1.49e391bd2143ep-6},
    {-0x1.c7545aa8c0dadp-1, 0x1.6cdfe10bba379p-6},
    {-0x1.bb6445eadae2cp-1, 0x1.8efea346845aep-6},
    {-0x1.ae66f68eedbc6p-1, 0x1.b02b2071c0c24p-6},
    {-0x1.a0644fb6d8db8p-1, 0x1.d05133c3af976p-6},
    {-0x1.9164d335425e2p-1, 0x1.ef5d57d53b4a7p-6},
    {-0x1.81719c62ec68ep-1, 0x1.069e593b92362p-5},
    {-0x1.70945a96f12c3p-1, 0x1.14ee9010d92e2p-5},
    {-0x1.5ed74b4532f83p-1, 0x1.22969f7b5c8c0p-5},
    {-0x1.4c4533c68b412p-1, 0x1.2f8e3ca7574ecp-5},
    {-0x1.38e95ace7b3c3p-1, 0x1.3bcd87e50de17p-5},
    {-0x1.24cf81925487fp-1, 0x1.474d117092814p-5},
    {-0x1.1003dca600f34p-1, 0x1.5205ddf5a36d5p-5},
    {-0x1.f52619257c3a1p-2, 0x1.5bf16accdf42fp-5},
    {-0x1.c9142c5898fc5p-2, 0x1.6509b1efb8df0p-5},
    {-0x1.9becb55272c9dp-2, 0x1.6d492da0c250dp-5},
    {-0x1.6dcb1f0620fffp-2, 0x1.74aadbc614fafp-5},
    {-0x1.3ecb6c46c76cbp-2, 0x1.7b2a40f3ccdd4p-5},
    {-0x1.0f0a26c56e49cp-2, 0x1.80c36b24bdd16p-5},
    {-0x1.bd489b79ec83bp-3, 0x1.8572f41fbb52cp-5},
    {-0x1.5b6e88ad5c00ep-3, 0x1.89360387fe3aap-5},
    {-0x1.f182ff48e8a27p-4, 0x1.8c0a5097676bap-5},
    {-0x1.2afad5ee95ad0p-4, 0x1.8dee238192cd4p-5},
    {-0x1.8ef487a8cbc32p-6, 0x1.8ee0567ee2e54p-5},
    {0x1.8ef487a8cbc32p-6, 0x1.8ee0567ee2e54p-5},
    {0x1.2afad5ee95ad0p-4, 0x1.8dee238192cd4p-5},
    {0x1.f182ff48e8a27p-4, 0x1.8c0a5097676bap-5},
    {0x1.5b6e88ad5c00ep-3, 0x1.89360387fe3aap-5},
    {0x1.bd489b79ec83bp-3, 0x1.8572f41fbb52cp-5},
    {0x1.0f0a26c56e49cp-2, 0x1.80c36b24bdd16p-5},
    {0x1.3ecb6c46c76cbp-2, 0x1.7b2a40f3ccdd4p-5},
    {0x1.6dcb1f0620fffp-2, 0x1.74aadbc614fafp-5},
    {0x1.9becb55272c9dp-2, 0x1.6d492da0c250dp-5},
    {0x1.c9142c5898fc5p-2, 0x1.6509b1efb8df0p-5},
    {0x1.f52619257c3a1p-2, 0x1.5bf16accdf42fp-5},
    {0x1.1003dca600f34p-1, 0x1.5205ddf5a36d5p-5},
    {0x1.24cf81925487fp-1, 0x1.474d117092814p-5},
    {0x1.38e95ace7b3c3p-1, 0x1.3bcd87e50de17p-5},
    {0x1.4c4533c68b412p-1, 0x1.2f8e3ca7574ecp-5},
    {0x1.5ed74b4532f83p-1, 0x1.22969f7b5c8c0p-5},
    {0x1.70945a96f12c3p-1, 0x1.14ee9010d92e2p-5},
    {0x1.81719c62ec68ep-1, 0x1.069e593b92362p-5},
    {0x1.9164d335425e2p-1, 0x1.ef5d57d53b4a7p-6},
    {0x1.a0644fb6d8db8p-1, 0x1.d05133c3af976p-6},
    {0x1.ae66f68eedbc6p-1, 0x1.b02b2071c0c24p-6},
    {0x1.bb6445eadae2cp-1, 0x1.8efea346845aep-6},
    {0x1.c7545aa8c0dadp-1, 0x1.6cdfe10bba379p-6},
    {0x1.d22ff5221288ap-1, 0x1.49e391bd2143ep-6},
    {0x1.dbf07d935a5afp-1, 0x1.261ef40a7a2dbp-6},
    {0x1.e490081f2891bp-1, 0x1.01a7c0a5c98e8p-6},
    {0x1.ec09586b58faap-1, 0x1.b9283b35df9afp-7},
    {0x1.f257e4db5aabcp-1, 0x1.6df524de84ee7p-7},
    {0x1.f777d976cfadap-1, 0x1.21e400109d579p-7},
    {0x1.fb661ac8c85a9p-1, 0x1.aa46b24145fd3p-8},
    {0x1.fe204ab274eccp-1, 0x1.0fc7ac3ac343cp-8},
    {0x1.ffa4e911f7533p-1, 0x1.d379f1845dc3ap-10},
};

__device__ __forceinline__ double cp_wave_sum(double x)
{
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) x = x + __shfl_xor(x, sh);
    return x;
}
__device__ __forceinline__ double cp_wave_max(double x)
{
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) x = fmax(x, __shfl_xor(x, sh));
    return x;
}

// The encounter frame of the relative position d = pb - pa and velocity w = vb - va: the speed wn = |w|, e_w along w, the miss
// m = d - (d . e_w) e_w and its length mn, e_1 along m, e_2 = e_w x e_1.  MPCX_ST_NUMERIC (only wn written) when wn is not positive
// and finite.
__device__ __forceinline__ int cp_frame(const double (&d)[3], const double (&w)[3], double &wn, double (&ew)[3], double &mn, double (&e1)[3],
                                        double (&e2)[3])
{
    wn = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    if (!(wn > 0.0) || !cp_finite(wn)) return MPCX_ST_NUMERIC;
    double m[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) ew[c] = w[c] / wn;
    const double dw = d[0] * ew[0] + d[1] * ew[1] + d[2] * ew[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) m[c] = d[c] - dw * ew[c];
    mn = sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2]);
    if (mn > 0.0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) e1[c] = m[c] / mn;
    } else {
        // the coordinate axis on which |e_w| is smallest (the first of equal ones), made orthogonal to e_w
        int ax = 0;
        double ea = ew[0];
        if (fabs(ew[1]) < fabs(ea)) { ax = 1; ea = ew[1]; }
        if (fabs(ew[2]) < fabs(ea)) { ax = 2; ea = ew[2]; }
#pragma unroll
        for (int c = 0; c < 3; ++c) e1[c] = (c == ax ? 1.0 : 0.0) - ea * ew[c];
        const double en = sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]);
#pragma unroll
        for (int c = 0; c < 3; ++c) e1[c] = e1[c] / en;
    }
    e2[0] = ew[1] * e1[2] - ew[2] * e1[1];
    e2[1] = ew[2] * e1[0] - ew[0] * e1[2];
    e2[2] = ew[0] * e1[1] - ew[1] * e1[0];
    return MPCX_ST_OK;
}

// The combined covariance in the encounter plane, C_2 = E^T Cs E with Cs = (c00, c01, c02, c11, c12, c22) and E = [e_1 e_2], and its
// eigenvalues l1 >= l2 (the smaller one as det / l1: no cancellation).  MPCX_ST_NUMERIC when they are not positive and finite.
struct CpPlane {
    double c11, c12, c22, l1, l2, det;
};
__device__ __forceinline__ int cp_plane_covariance(const double (&Cs)[6], const double (&e1)[3], const double (&e2)[3], CpPlane &pl)
{
    double g1[3], g2[3];                                             // Cs e1, Cs e2
    g1[0] = Cs[0] * e1[0] + Cs[1] * e1[1] + Cs[2] * e1[2];
    g1[1] = Cs[1] * e1[0] + Cs[3] * e1[1] + Cs[4] * e1[2];
    g1[2] = Cs[2] * e1[0] + Cs[4] * e1[1] + Cs[5] * e1[2];
    g2[0] = Cs[0] * e2[0] + Cs[1] * e2[1] + Cs[2] * e2[2];
    g2[1] = Cs[1] * e2[0] + Cs[3] * e2[1] + Cs[4] * e2[2];
    g2[2] = Cs[2] * e2[0] + Cs[4] * e2[1] + Cs[5] * e2[2];
    const double c11 = e1[0] * g1[0] + e1[1] * g1[1] + e1[2] * g1[2];
    const double c12 = e1[0] * g2[0] + e1[1] * g2[1] + e1[2] * g2[2];
    const double c22 = e2[0] * g2[0] + e2[1] * g2[1] + e2[2] * g2[2];
    const double tr = c11 + c22, df = c11 - c22;
    const double l1 = 0.5 * (tr + sqrt(df * df + 4.0 * c12 * c12));
    const double det = c11 * c22 - c12 * c12;
    const double l2 = det / l1;
    pl = CpPlane{c11, c12, c22, l1, l2, det};
    return !(l2 > 0.0) || !cp_finite(l2) || !cp_finite(l1) ? MPCX_ST_NUMERIC : MPCX_ST_OK;
}

// what the adjoint sweep and the passes over the nodes need of one manoeuvring object (wave-uniform)
struct CpMover {
    int o, k, nn;                     // the object, the interval the encounter falls in, its node count
    double hn, htau, L, cfac;         // node spacing in s and in the object's own time unit; its length unit; (L / Tu^2): c_m = cfac / mass_m
    const double *mass;               // Y[o][6][.]
};

// The object cp_state placed at `nd` as a mover -- one of the constellation: the row side, whose rows are K long.  MPCX_ST_BADK when
// its span and time unit give no positive finite tf (the linearisation ran with tf = 1), otherwise the discretiser's status.
__device__ __forceinline__ int cp_mover(const CpSide &row, const int32_t *dstat, const CpNode &nd, size_t K, CpMover &mv)
{
    int st = MPCX_ST_OK;
    const double L = row.units[2 * nd.o], Tu = row.units[2 * nd.o + 1];
    double tfv;
    if (!tr_tf(row.span[2 * nd.o], row.span[2 * nd.o + 1], Tu, tfv)) st = MPCX_ST_BADK;
    else if (dstat[nd.o] != MPCX_ST_OK) st = dstat[nd.o];
    mv = CpMover{nd.o, nd.k, nd.nn, nd.hn, tfv / (double)(nd.nn - 1), L, L / (Tu * Tu), row.Y + ((size_t)nd.o * 7 + 6) * K};
    return st;
}

// R Lam of the two nodes that bracket the encounter, entry (lr, lc): sgn [e_1 e_2 e_w]^T L [hp I | h_tau hv I | 0] with the Hermite
// basis (h01, h11) of the upper node in seed_hi and (h00, h10) of the lower one in seed_lo
__device__ __forceinline__ void cp_sweep_seed(double sgn, const double (&e1)[3], const double (&e2)[3], const double (&ew)[3], double L, double ht,
                                              double h00, double h10, double h01, double h11, int lr, int lc, double &seed_hi, double &seed_lo)
{
    double Rv[3];
#pragma unroll
    for (int x = 0; x < 3; ++x) Rv[x] = sgn * (lr == 0 ? e1[x] : (lr == 1 ? e2[x] : ew[x]));
    const int cc = lc < 3 ? lc : lc - 3;
    const double Rc = cc == 0 ? Rv[0] : (cc == 1 ? Rv[1] : Rv[2]);
    if (lc < 3) { seed_hi = (L * h01) * Rc; seed_lo = (L * h00) * Rc; }
    else if (lc < 6) { seed_hi = (L * (ht * h11)) * Rc; seed_lo = (L * (ht * h10)) * Rc; }
}

// One node q of the adjoint sweep on the node's record rec = A | B_kn | B_kp and the rows lam = lam_q+1.  A lane that owns entry
// (gr, gc) of g_m forms gn = lam B_kn and gp = lam B_kp there, stores g_q+1 = lam_q+2 B_kn[q+1] + lam_q+1 B_kp[q] to *gq -- `carry`
// is the first term, absent at the node the sweep starts from (`first`) -- and keeps gn as the next carry.  A lane that owns entry
// (lr, lc) of lam gets lam_q = lam_q+1 A_q back (plus seed_lo at the first node); the caller stores it behind its barrier.
__device__ __forceinline__ double cp_sweep_node(const double *lam, const double *rec, bool first, bool has_g, int gr, int gc, double *gq,
                                                double &carry, bool has_lam, int lr, int lc, double seed_lo)
{
    double lnew = 0.0;
    if (has_g) {
        double gn = lam[gr * 7] * rec[49 + gc], gp = lam[gr * 7] * rec[70 + gc];
#pragma unroll
        for (int x = 1; x < 7; ++x) {
            gn = gn + lam[gr * 7 + x] * rec[49 + x * 3 + gc];
            gp = gp + lam[gr * 7 + x] * rec[70 + x * 3 + gc];
        }
        *gq = first ? gp : carry + gp;
        carry = gn;
    }
    if (has_lam) {
        lnew = lam[lr * 7] * rec[lc];
#pragma unroll
        for (int x = 1; x < 7; ++x) lnew = lnew + lam[lr * 7 + x] * rec[x * 7 + lc];
        if (first) lnew = lnew + seed_lo;
    }
    return lnew;
}

enum { CP_REC = 91, CP_REC_PAD = 96 };                               // a record's A | B_kn | B_kp, and its room in LDS

// The adjoint sweep for NR rows, run by one wave: lam_kme+1 = seed_hi, lam_kme = lam_kme+1 A_kme + seed_lo, lam_q = lam_q+1 A_q;
// g_q+1 = lam_q+2 B_kn[q+1] + lam_q+1 B_kp[q], g_0 = lam_1 B_kn[0], written to g[(row * 3 + component) * K + node] for the nodes
// 0 .. kme + 1.  Lane e < 7 NR owns entry e of lam, lane e < 3 NR entry e of g_m; a node's record is fetched one node ahead of its
// arithmetic.  Called by the whole wave; ends with a barrier (g is read back by other lanes).
template <int NR>
__device__ __forceinline__ void aj_sweep(int lane, const double *srec, int kme, double seed_hi, double seed_lo, double *g, size_t K,
                                         double *rec, double *lam)
{
    constexpr int NL = NR * 7, NG = NR * 3;
    const int lr = lane < NL ? lane / 7 : 0, lc = lane < NL ? lane - 7 * (lane / 7) : 0;
    const int gr = lane < NG ? lane / 3 : 0, gc = lane < NG ? lane - 3 * (lane / 3) : 0;
    if (lane < NL) lam[lane] = seed_hi;
    double r0 = 0.0, r1 = 0.0;                                       // the record in flight: entries lane, lane + 64 (< 91)
    {
        const double *rp = srec + (size_t)kme * MPCX_STAGE_DOUBLES;
        r0 = rp[lane];
        if (lane + 64 < CP_REC) r1 = rp[lane + 64];
    }
    double carry = 0.0;                                              // lam_q+2 B_kn[q+1], entry (gr, gc)
    for (int q = kme; q >= 0; --q) {
        rec[lane] = r0;
        if (lane + 64 < CP_REC) rec[lane + 64] = r1;
        __syncthreads();
        if (q >= 1) {                                                // the next node's record, ahead of this node's arithmetic
            const double *rp = srec + (size_t)(q - 1) * MPCX_STAGE_DOUBLES;
            r0 = rp[lane];
            if (lane + 64 < CP_REC) r1 = rp[lane + 64];
        }
        const double lnew = cp_sweep_node(lam, rec, q == kme, lane < NG, gr, gc, g + (size_t)lane * K + q + 1, carry, lane < NL, lr, lc, seed_lo);
        __syncthreads();
        if (lane < NL) lam[lane] = lnew;                             // lam_q
    }
    if (lane < NG) g[(size_t)lane * K] = carry;                      // g_0 = lam_1 B_kn[0]
    __syncthreads();
}

}  // namespace mpcx
