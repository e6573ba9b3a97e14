// integrator_device.hpp -- scipy's adaptive Runge-Kutta driver (scipy/integrate/_ivp/rk.py, common.py) as propagate_kernel and
// discretize_kernel share it: the tableaux, the initial step, the step prologue, the step size after an accepted and after a
// rejected attempt, and the dense output.  Scalar arithmetic for the host and the device (tests/tools/rk_step_factor_check.cpp
// compiles the controller on the host); the kernels' stage loops, error norms and accept branches are their own.
// Included by mpcx_device.hpp.
#pragma once
#include <hip/hip_runtime.h>

namespace mpcx {

// Dormand-Prince 5(4) tableau as used by scipy's RK45 (scipy/integrate/_ivp/rk.py:377-404)
__device__ constexpr double RK_C[6] = {0.0, 1.0 / 5, 3.0 / 10, 4.0 / 5, 8.0 / 9, 1.0};
__device__ constexpr double RK_A[6][5] = {
    {0, 0, 0, 0, 0},
    {1.0 / 5, 0, 0, 0, 0},
    {3.0 / 40, 9.0 / 40, 0, 0, 0},
    {44.0 / 45, -56.0 / 15, 32.0 / 9, 0, 0},
    {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729, 0},
    {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656}};
__device__ constexpr double RK_B[6] = {35.0 / 384, 0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784,
                                       11.0 / 84};
__device__ constexpr double RK_E[7] = {-71.0 / 57600, 0, 71.0 / 16695, -71.0 / 1920,
                                       17253.0 / 339200, -22.0 / 525, 1.0 / 40};
__device__ constexpr double RK_P[7][4] = {
    {1, -8048581381.0 / 2820520608, 8663915743.0 / 2820520608, -12715105075.0 / 11282082432},
    {0, 0, 0, 0},
    {0, 131558114200.0 / 32700410799, -68118460800.0 / 10900136933, 87487479700.0 / 32700410799},
    {0, -1754552775.0 / 470086768, 14199869525.0 / 1410260304, -10690763975.0 / 1880347072},
    {0, 127303824393.0 / 49829197408, -318862633887.0 / 49829197408,
     701980252875.0 / 199316789632},
    {0, -282668133.0 / 205662961, 2019193451.0 / 616988883, -1453857185.0 / 822651844},
    {0, 40617522.0 / 29380423, -110615467.0 / 29380423, 69997945.0 / 29380423}};
constexpr double RK_SAFETY = 0.9, RK_MIN_FACTOR = 0.2, RK_MAX_FACTOR = 10.0;
// scipy's RK23 (Bogacki-Shampine 3(2), rk.py:183-278; Discretizer.ivp_solver = 'RK23'): C = (0, 1/2, 3/4), A, B, E, P (4 x 3)
__device__ constexpr double RK23_C[3] = {0.0, 1.0 / 2, 3.0 / 4};
__device__ constexpr double RK23_A10 = 1.0 / 2, RK23_A21 = 3.0 / 4;      // (A[2][0] = 0)
__device__ constexpr double RK23_B[3] = {2.0 / 9, 1.0 / 3, 4.0 / 9};
__device__ constexpr double RK23_E[4] = {5.0 / 72, -1.0 / 12, -1.0 / 9, 1.0 / 8};
__device__ constexpr double RK23_P[4][3] = {{1, -4.0 / 3, 5.0 / 9}, {0, 1, -2.0 / 3}, {0, 4.0 / 3, -8.0 / 9}, {0, -1, 1}};

// rk.py:93: error_exponent = -1 / (error_estimator_order + 1) (METHOD 45: -1/5, METHOD 23: -1/3) -- of the step factor after an
// accepted and after a rejected attempt, and, negated, of select_initial_step's h1
template <int METHOD>
constexpr double rk_error_exponent = (METHOD == 23) ? -1.0 / 3.0 : -0.2;
// select_initial_step (scipy common.py:68-134, direction +1) in two parts, around the right-hand side at y + h0 f that d2 is
// measured on.  d0, d1, d2: the scaled norms of y, f and (f(y + h0 f) - f) / h0; interval: |t_bound - t|.
__host__ __device__ __forceinline__ double rk_initial_h0(double d0, double d1, double interval)
{
    const double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
    return fmin(h0, interval);
}
template <int METHOD>
__host__ __device__ __forceinline__ double rk_initial_h_abs(double h0, double d1, double d2, double interval, double max_step)
{
    double h1;
    if (d1 <= 1e-15 && d2 <= 1e-15) h1 = fmax(1e-6, h0 * 1e-3);
    else h1 = pow(0.01 / fmax(d1, d2), -rk_error_exponent<METHOD>);
    const double h_abs = fmin(fmin(100.0 * h0, h1), fmin(interval, max_step));
    return (interval == 0.0) ? 0.0 : h_abs;
}

// The opening of an attempted step (rk.py:110-135, direction +1): h_abs clamped to [min_step, max_step] unless the attempt
// before was rejected, the step cut at t_bound.  too_small: scipy's TOO_SMALL_STEP (a non-finite h_abs as well).  min_step is the
// caller's: 10 |nextafter(t, inf) - t|, which the rollout evaluates only where h_abs could be near it.
struct RkAttempt {
    double h, t_new, h_try;
    bool too_small;
};
__host__ __device__ __forceinline__ RkAttempt rk_attempt(double t, double t_bound, double max_step, bool rejected, double &h_abs, double min_step)
{
    if (!rejected) {
        if (h_abs > max_step) h_abs = max_step;
        else if (h_abs < min_step) h_abs = min_step;
    }
    RkAttempt s;
    s.too_small = !(h_abs >= min_step);
    s.t_new = t + h_abs;
    if (s.t_new - t_bound > 0.0) s.t_new = t_bound;
    s.h = s.t_new - t;
    s.h_try = fabs(s.h);
    return s;
}

// scipy's step-size controller after an ACCEPTED step (rk.py:149-156): the step size h_abs that the next step starts from,
//   h_try * factor,  factor = min(RK_MAX_FACTOR, RK_SAFETY * error_norm^(-1 / (q + 1))),  after a rejection min(1, factor)
// (METHOD 45: q + 1 = 5, METHOD 23: q + 1 = 3; error_norm < 1) -- with the pow evaluated only where its value decides something.
// The caller's next step clamps what this returns to [min_step, max_step] before anything reads it, and after that clamp the
// result is the formula's, bit for bit:
//  (a) at_bound: the step ended on the integration's end point.  No further step: h_abs stays what it is.
//  (b) error_norm < 2^-18 (RK45; 2^-11 for RK23): RK_SAFETY * error_norm^(..) >= 10.9 (11.4) > RK_MAX_FACTOR with a margin no
//      rounding of pow comes near, so factor = RK_MAX_FACTOR exactly.
//  (c) not after a rejection, and error_norm * max_step^5 < (RK_SAFETY h_try)^5 / 2 (^3 for RK23), which is
//      error_norm (max_step / (RK_SAFETY h_try))^5 < 1/2 without the division: then h_try RK_SAFETY error_norm^(-1/5) exceeds
//      max_step by the factor 2^(1/5) = 1.15 (2^(1/3) = 1.26) at least, against relative errors of 1e-15 in both products and in
//      pow.  With error_norm >= 2^-18 the bound also gives max_step / h_try < 0.9 * 2^(17/5) = 9.5 (0.9 * 2^(10/3) = 9.1) < RK_MAX_FACTOR,
//      so h_try * factor > max_step on either side of the min, and the next step's clamp makes it max_step: any value above
//      max_step does (not max_step itself, which would take the clamp's other arm).  The comparison is trusted only with
//      (RK_SAFETY h_try)^5 far inside the normal range, where neither side can have lost its value to overflow or underflow.
//  (d) otherwise: the formula.
// Per lane; the pow is behind a branch of its own, which a wave with no lane in (d) skips.
template <int METHOD>
__host__ __device__ __forceinline__ double rk_accepted_h_abs(double h_abs, double error_norm, double h_try, double max_step,
                                                             bool rejected, bool at_bound)
{
    constexpr double kSmall = (METHOD == 23) ? 0x1p-11 : 0x1p-18;
    if (at_bound) return h_abs;
    double factor = RK_MAX_FACTOR;
    if (!(error_norm < kSmall)) {
        if (!rejected) {
            const double sh = RK_SAFETY * h_try;
            const double m2 = max_step * max_step, s2 = sh * sh;
            const double mp = (METHOD == 23) ? m2 * max_step : (m2 * m2) * max_step;
            const double sp = (METHOD == 23) ? s2 * sh : (s2 * s2) * sh;
            if (error_norm * mp < 0.5 * sp && sp > 1e-250 && sp < 1e250) return 2.0 * max_step;
        }
        factor = fmin(RK_MAX_FACTOR, RK_SAFETY * pow(error_norm, rk_error_exponent<METHOD>));
    }
    if (rejected) factor = fmin(1.0, factor);
    return h_try * factor;
}

// ... and after a REJECTED one (rk.py:157-160; error_norm >= 1, or NaN: the comparison that accepts is false for it, as in scipy)
template <int METHOD>
__host__ __device__ __forceinline__ double rk_rejected_h_abs(double h_try, double error_norm)
{
    return h_try * fmax(RK_MIN_FACTOR, RK_SAFETY * pow(error_norm, rk_error_exponent<METHOD>));
}

// Dense output (RkDenseOutput, rk.py:552-574): sol(t_old + x h) = y_old + h Q p(x), Q = K^T P, p(x) = (x, x^2, x^3[, x^4]).
// rk_dense_q: RK45's row of Q for one component from that component's column kk of K (f, the five inner stages, f(y_new)).  (RK23's
// row, which only discretize_kernel forms, is its own text there: through a function its uniform forms spill differently.)
// rk_dense_at: a row's polynomial q . p(x), RK23's without x^4; the caller forms h (q . p) + y_old.
__device__ __forceinline__ void rk_dense_q(const double (&kk)[7], double (&q)[4])
{
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < 7; ++j) s += kk[j] * RK_P[j][cc];
        q[cc] = s;
    }
}
template <int METHOD>
__host__ __device__ __forceinline__ double rk_dense_at(const double (&q)[4], double x)
{
    const double p1 = x, p2 = p1 * x, p3 = p2 * x, p4 = p3 * x;
    return (METHOD == 23) ? q[0] * p1 + q[1] * p2 + q[2] * p3 : q[0] * p1 + q[1] * p2 + q[2] * p3 + q[3] * p4;
}

}  // namespace mpcx
