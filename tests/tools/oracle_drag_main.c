/*
 * tests/tools/oracle_drag_main.c -- a stand-alone caller of the oracle's drag / atmosphere entry points (oracle/mpc_oracle.h: the
 * *_atm functions) on the floor-crossing case of tests/drag_cases.py (350 x 700 km, floor at 500 km, K = 6, tf = 1), for a run of
 * the oracle's C under the host sanitizers without Python in the process:
 *   cc -O1 -g -std=gnu11 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Ioracle tests/tools/oracle_drag_main.c <the .c files of oracle/> -lm
 * Prints two sums and compares them with the values of the ordinary build; exit status 0 when they agree to 1e-9 relative.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include "mpc_oracle.h"

enum { K = 6 };
static const double X[42] = {0.5275869865481799, 0.8832152558804939, -0.037124300068152156, -0.9206772876021297, -0.5824881301118816, 0.527734631414968, -0.5665111107797445, 0.4192296174651201, 0.7980747533594179, 0.057769180138633386, -0.7676393338052006, -0.5671138639584096, -0.6330222215594891, -0.06439816585516416, 0.5969885170118686, 0.42608799668980546, -0.3193351587515463, -0.6331491802242103, 4.869040697224311, -1.886551624990698, -5.969359650065252, -1.7541363764546365, 4.712306032700155, 4.92521116666329, 3.9148558118950665, 4.572885438056508, -1.271852552141161, -5.1183145049018, -2.0691541249766594, 3.857226450323184, 0.8020485464293371, 4.123040965658531, 1.5712337017503077, -3.0113191642523756, -3.473684713309478, 0.7738610136309, 1.0, 0.9963369441366228, 0.9882357981329981, 0.9761600986860546, 0.9708049591175419, 0.9653498320109514};
static const double U[18] = {0.04277699642047284, -0.05708375568864456, 0.26544606897300976, -0.16085449528642096, 0.06617156616641691, -0.014342594397899665, -0.03545063884714269, 0.10663588121198411, -0.1817922000607549, -0.09846762100886533, -0.011416014445729657, 0.17412738366841587, 0.008904687115378083, 0.08956882370088885, -0.18633059650275363, -0.12388875452076326, 0.09695294734242305, -0.06281797400433668};
static const double CST[8] = {39.47841760435744, 0.9285380722101152, 0.00108262668, 45.72549500786051, 0.0883989668924858, 1.1776261542589513e-08, 6861323.397150194, 3.7769058764115426e-17};
static const double Y0[7] = {0.5275869865481799, -0.5665111107797445, -0.6330222215594891, 4.869040697224311, 3.9148558118950665, 0.8020485464293371, 1.0};
static const double ATM[4] = {61.94665395952502, -6.828, 0.0, 500000.0};
static const double WANT_A = 328.0008069705121, WANT_Y = 244.6658388088252;

int main(void)
{
    const int flags = ORACLE_FLAG_DRAG | ORACLE_FLAG_J2 | ORACLE_FLAG_ATMO;
    double f[7], A[49], xi[7], x0[7], u0[3];
    for (int i = 0; i < 7; ++i) x0[i] = X[i * K];
    for (int i = 0; i < 3; ++i) u0[i] = U[i * K];
    int rc = oracle_dynamics_atm(x0, u0, 1.0, CST, flags, ATM, f);
    oracle_A_func_atm(x0, u0, 1.0, CST, flags, ATM, A);
    oracle_xi_func_atm(x0, u0, 1.0, CST, flags, ATM, xi);
    /* exact-size heap buffers: an overrun by one element is a sanitizer report */
    double *Ak = malloc((K - 1) * 49 * sizeof(double)), *Bp = malloc((K - 1) * 21 * sizeof(double)), *Bn = malloc((K - 1) * 21 * sizeof(double));
    double *Sg = malloc(7 * (K - 1) * sizeof(double)), *Xi = malloc(7 * (K - 1) * sizeof(double));
    int32_t *cnt = malloc((K - 1) * sizeof(int32_t)), *nfev = malloc((K - 1) * sizeof(int32_t));
    const int cap = 64 * (K - 1);
    double *nt = malloc(cap * sizeof(double)), *ny = malloc((size_t)cap * 56 * sizeof(double));
    rc |= oracle_discretize_mode_atm(K, K, X, U, 1.0, CST, flags, ATM, 1e-2, 0, Ak, Bp, Bn, Sg, Xi, cnt, nfev, nt, ny, cap);
    rc |= oracle_discretize_mode_atm(K, K, X, U, 1.0, CST, flags | 8, ATM, 1e-2, 0, Ak, Bp, Bn, Sg, Xi, cnt, nfev, 0, 0, 0);      /* RK23 */
    rc |= oracle_discretize_mode_atm(K, K, X, U, 1.0, CST, flags, ATM, 1e-2, 11, Ak, Bp, Bn, Sg, Xi, cnt, nfev, 0, 0, 0);         /* uniform steps */
    rc |= oracle_discretize_mode_atm(K, K, X, U, 1.0, CST, flags, ATM, 1e-2, 0, Ak, Bp, Bn, Sg, Xi, 0, 0, 0, 0, 0);
    double sa = 0.0, sy = 0.0;
    for (int i = 0; i < (K - 1) * 49; ++i) sa += fabs(Ak[i]);
    oracle_ctrl ctrl = {ORACLE_CTRL_SEQUENCE, {0.0, 0.0, 0.0}, U, K, 1.0};
    double *y = malloc(7 * 20 * sizeof(double));
    int32_t ns = 0;
    rc |= oracle_propagate_atm(Y0, 1.0, CST, flags, ATM, &ctrl, 20, 1e-3, y, &ns);
    for (int i = 0; i < 7 * 20; ++i) sy += fabs(y[i]);
    printf("status %d, sum|A| %.17g (want %.17g), sum|y| %.17g (want %.17g), %d steps\n", rc, sa, WANT_A, sy, WANT_Y, (int)ns);
    int ok = rc == 0 && fabs(sa - WANT_A) <= 1e-9 * WANT_A && fabs(sy - WANT_Y) <= 1e-9 * WANT_Y && isfinite(f[3] + A[24] + xi[3]);
    free(Ak); free(Bp); free(Bn); free(Sg); free(Xi); free(cnt); free(nfev); free(nt); free(ny); free(y);
    return ok ? 0 : 1;
}
