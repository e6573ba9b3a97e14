// rk_step_factor_check -- host check of rk_accepted_h_abs (csrc/mpcx_device.hpp), the step-size controller's pow-free paths.
// Built as host code only, with -fsanitize=address,undefined, by tests/test_rk_step_factor_host.py.
//
// For every input the helper's value goes through the clamp that opens the integrators' next step (discretize.hip: `if (h_abs >
// max_step) h_abs = max_step; else if (h_abs < min_step) h_abs = min_step;`), and so does the plain formula of scipy's
// controller (rk.py:149-156); the two next step sizes must be the same bits.  A step that ended on the end point has no next
// step: there the helper must hand h_abs back untouched.  Prints the number of inputs per case (a)-(d) and of mismatches; exit
// status 1 on any mismatch or if a case was never reached.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../mpconstellation_amd/csrc/mpcx_device.hpp"

using namespace mpcx;

static uint64_t bits(double v) { uint64_t b; std::memcpy(&b, &v, 8); return b; }
static double ulps(double v, int n)
{
    for (int i = 0; i < std::abs(n); ++i) v = std::nextafter(v, n > 0 ? INFINITY : -INFINITY);
    return v;
}
static double clamp_next(double h_abs, double max_step, double min_step)
{
    if (h_abs > max_step) h_abs = max_step;
    else if (h_abs < min_step) h_abs = min_step;
    return h_abs;
}
template <int METHOD>
static double plain(double error_norm, double h_try, bool rejected)
{
    const double expo = (METHOD == 23) ? -1.0 / 3.0 : -0.2;
    double factor = (error_norm == 0.0) ? RK_MAX_FACTOR : std::fmin(RK_MAX_FACTOR, RK_SAFETY * std::pow(error_norm, expo));
    if (rejected) factor = std::fmin(1.0, factor);
    return h_try * factor;
}

static long n_case[4], n_bad;

template <int METHOD>
static void check(double en, double h_try, double max_step, bool rejected, double min_step)
{
    if (!(en < 1.0)) return;                                  // the accept branch
    const double small = (METHOD == 23) ? 0x1p-11 : 0x1p-18;
    const double sentinel = 0.12345;
    if (bits(rk_accepted_h_abs<METHOD>(sentinel, en, h_try, max_step, rejected, true)) != bits(sentinel)) {
        ++n_bad;
        std::printf("MISMATCH at_bound: method %d en %.17g h_try %.17g max_step %.17g rejected %d\n", METHOD, en, h_try, max_step, (int)rejected);
    }
    ++n_case[0];
    const double got = rk_accepted_h_abs<METHOD>(sentinel, en, h_try, max_step, rejected, false);
    const double want = plain<METHOD>(en, h_try, rejected);
    if (en < small) ++n_case[1];
    else if (bits(got) == bits(2.0 * max_step) && bits(got) != bits(want)) ++n_case[2];
    else ++n_case[3];
    const double a = clamp_next(got, max_step, min_step), b = clamp_next(want, max_step, min_step);
    if (bits(a) != bits(b)) {
        if (++n_bad <= 20)
            std::printf("MISMATCH: method %d en %.17g h_try %.17g max_step %.17g rejected %d: next step %.17g, formula %.17g\n",
                        METHOD, en, h_try, max_step, (int)rejected, a, b);
    }
}

template <int METHOD>
static void sweep()
{
    const int n = (METHOD == 23) ? 3 : 5;
    const double small = (METHOD == 23) ? 0x1p-11 : 0x1p-18;
    const double max_steps[] = {1e-2, 1.0, 1e-3, 0.37, INFINITY};
    const double ratios[] = {1.0, 1.0 - 0x1p-52, 0.9, 0.5, 1e-3};
    std::vector<double> ens;
    ens.push_back(0.0);
    for (int k = 0; k <= 3000; ++k) ens.push_back(std::pow(10.0, -300.0 + 0.1 * k));          // log grid 1e-300 .. 1
    std::vector<double> thr = {small, 1.0};
    // error norms at which RK_SAFETY en^expo crosses RK_MAX_FACTOR and 1 (where the min() arms of the formula change)
    thr.push_back(std::pow(RK_SAFETY / RK_MAX_FACTOR, (double)n));
    thr.push_back(std::pow(RK_SAFETY, (double)n));
    for (double max_step : max_steps) {
        for (double ratio : ratios) {
            const double h_try = std::isinf(max_step) ? ratio * 1e-2 : ratio * max_step;
            std::vector<double> all = ens, th = thr;
            // case (c)'s boundary for this ratio: en (max_step / (RK_SAFETY h_try))^n = 1/2, and where the formula itself reaches
            // max_step (twice that error norm)
            if (!std::isinf(max_step)) {
                const double q = RK_SAFETY * h_try / max_step;
                th.push_back(0.5 * std::pow(q, (double)n));
                th.push_back(std::pow(q, (double)n));
            }
            for (double t : th)
                for (int d = -8; d <= 8; ++d) all.push_back(ulps(t, d));
            for (double en : all)
                for (int rej = 0; rej < 2; ++rej)
                    for (double min_step : {0.0, 10.0 * 0x1p-53})
                        check<METHOD>(en, h_try, max_step, rej != 0, min_step);
        }
        if (std::isinf(max_step)) continue;
        // h_try / max_step that puts case (c) on its boundary for given error norms (beyond the five ratios above)
        for (double en : {small, 1e-5, 1e-4, 1e-3, 1e-2, 0.1, 0.5, 0.999}) {
            const double q = std::pow(2.0 * en, 1.0 / n) / RK_SAFETY;                        // h_try / max_step on the boundary
            for (int d = -8; d <= 8; ++d)
                for (int rej = 0; rej < 2; ++rej) check<METHOD>(en, ulps(q * max_step, d), max_step, rej != 0, 0.0);
        }
    }
}

int main()
{
    sweep<45>();
    sweep<23>();
    std::printf("cases: at_bound %ld, small %ld, above_max_step %ld, pow %ld; mismatches %ld\n", n_case[0], n_case[1], n_case[2], n_case[3], n_bad);
    const bool reached = n_case[0] > 0 && n_case[1] > 0 && n_case[2] > 0 && n_case[3] > 0;
    if (!reached) std::printf("a case was never reached\n");
    return (n_bad == 0 && reached) ? 0 : 1;
}
