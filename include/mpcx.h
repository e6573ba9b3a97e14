/*
 * mpcx.h -- C ABI of libmpcx.so, the MI355X (gfx950) batched constellation-MPC engine.
 *
 * The reference (rgovindjee/mpconstellation) has no FFI layer: its hot path is two Python
 * classes.  Each entry point below names the reference interface it replaces (file:line into
 * the reference repo); mpconstellation_amd/_ffi.py is the ctypes binding a maintainer of the
 * reference would add.
 *
 * Conventions
 *  - plain C, fp64 everywhere, row-major (numpy C-order) arrays, satellite index outermost;
 *  - every function returns 0 on success or a negative MPCX_E_* code; mpcx_last_error() gives
 *    the text; per-satellite outcomes come back in int32 status arrays (MPCX_ST_*);
 *  - "_dev" variants take DEVICE pointers (HBM resident) and enqueue on `stream` (a hipStream_t
 *    passed as void*, NULL = default stream) without synchronising; the others take HOST
 *    pointers, stage through HBM and return when the results are in the caller's buffers;
 *  - the library never keeps a caller pointer after a call returns (host variants) or after
 *    the enqueued work has completed (device variants);
 *  - there is no CPU fallback: without a HIP device mpcx_create fails with MPCX_E_NODEVICE;
 *  - the solver's problem options are one mpcx_solve_opts per call or, in the *_sat entry points, one row per satellite of a
 *    table popts [S][MPCX_NPOPT] (MPCX_PO_*): a constellation with different limits per satellite is still one launch.
 */
#ifndef MPCX_H
#define MPCX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPCX_VERSION 500

/* return codes */
#define MPCX_OK 0
#define MPCX_E_NODEVICE (-1)
#define MPCX_E_BADARG (-2)
#define MPCX_E_HIP (-3)
#define MPCX_E_NOMEM (-4)

/* per-satellite status */
#define MPCX_ST_OK 0
#define MPCX_ST_MASS 1        /* mass <= 0 in the dynamics (reference raises, simulator.py:135-136) */
#define MPCX_ST_STEP 2        /* RK45 step size underflow (scipy: "Required step size is less than spacing") */
#define MPCX_ST_FOH 3         /* FOH index outside the input table (reference: IndexError) */
#define MPCX_ST_SINGULAR 4    /* state-transition matrix not invertible (np.linalg.inv raises) */
#define MPCX_ST_MAXITER 5     /* solver hit max_iter without meeting tol */
#define MPCX_ST_NUMERIC 6     /* solver: non-finite value or factorisation breakdown */
#define MPCX_ST_ACCEPTABLE 7  /* solver stopped at the 'acceptable' level (ipopt acceptable_tol) */
#define MPCX_ST_BADK 9        /* ragged batch: this satellite's node / table-column / output-point count is outside the range
                               * the call accepts (solve: 3..K, discretize: 2..K, propagate: 1..n_eval, tables: 2..Ku) */
#define MPCX_ST_INFEASIBLE 8  /* solver: the constraint set is empty whatever the dynamics (start node outside its own radius
                               * bounds, terminal window outside r_max, r_min > r_max, empty window or tf range); seen before
                               * the first iteration: x_bar, u_bar, tf_bar come back, kkt = the violation (ipopt: restoration
                               * failure / "converged to a point of local infeasibility", ignored by optimizer.py:603) */
#define MPCX_ST_TIMEOUT 10    /* time-parallel solve only (MPCX_SOLVE_TIME_PARALLEL): one of the satellite's workgroups did not answer
                               * within the wait limit (~0.1 s of polling) -- e.g. another long kernel kept it from becoming
                               * resident; not a numerical failure: X, U, NU hold the last iterate, kkt = -1; solve again
                               * without the flag or with the device to itself */

/* dynamics flags (reference include_drag / include_J2 keyword arguments).  On the discretize / mpc_step entry points
 * MPCX_FLAG_DRAG is the reference's Discretizer(include_drag=True) (linearize_discretize.py:162-173) with the simulator's
 * atmosphere -- the fixed density 9.983e-13 kg/m^3 over the constants' RHO, drho = 0, C_D = 2.5: the drag partials in A
 * (velocity block, mass column), and drag in Sigma and xi.  MPCX_FLAG_ATMO (below) replaces that atmosphere by an
 * altitude-dependent one. */
#define MPCX_FLAG_DRAG 1
#define MPCX_FLAG_J2 2
/* discretize entry points only: Discretizer.use_uniform_steps (linearize_discretize.py:27-30, 50-53) with
 * integrator_steps = n: flags |= MPCX_FLAG_UNIFORM_STEPS | MPCX_UNIFORM_STEPS(n).  The quadrature then runs over n uniform
 * points per interval of the RK45 dense output instead of the accepted step nodes. */
#define MPCX_FLAG_UNIFORM_STEPS 4
#define MPCX_UNIFORM_STEPS(n) ((n) << 8)
/* discretize entry points only: Discretizer.ivp_solver = 'RK23' (linearize_discretize.py:40,105: the attribute is solve_ivp's
 * `method`) -- scipy's Bogacki-Shampine 3(2) pair instead of the default 'RK45', same step-size controller, same tolerances.
 * The implicit methods scipy also offers (Radau, BDF, LSODA) and DOP853 are not implemented. */
#define MPCX_FLAG_RK23 8
/* mpcx_mpc_update_batch's disc_flags only: the planning rollouts -- the tangential reference rollout and the re-rollouts under
 * the optimised sequence -- use the dynamics of the discretisation, disc_flags & (MPCX_FLAG_DRAG | MPCX_FLAG_J2), so that the
 * planner predicts what that model flies.  Without it they use neither (flags 0), as the reference's run_nonlinear does
 * (control.py:237-240).  The discretize entry points ignore the bit. */
#define MPCX_FLAG_PLAN_ROLLOUTS 16
/* With MPCX_FLAG_DRAG, wherever that flag is honoured -- the propagate, discretize / stage, fused-step, scp_iteration (both flag
 * words) and mpc_update (disc_flags, passed on to the planning rollouts by MPCX_FLAG_PLAN_ROLLOUTS, and sim_flags) entry points:
 * the drag uses the context's altitude-dependent atmosphere (mpcx_set_atmosphere below) instead of the fixed density.  The
 * density at a stage's own altitude enters every right-hand side, Sigma and xi, and the linearisation gains the position block
 * Dr a_D = -C_D S / (2 m) |v| v (drho r_hat^T) (linearize_discretize.py:164-166: the reference's rho_func / drho_func).  The bit
 * without MPCX_FLAG_DRAG, or on a context with no atmosphere set, is MPCX_E_BADARG before anything is enqueued.  Without the
 * bit every call takes the kernels it takes on a context that never had an atmosphere. */
#define MPCX_FLAG_ATMO 32
/* mpcx_discretize_stages_dev and mpcx_discretize_stages_ragged_dev only, with MPCX_FLAG_DRAG and the adaptive RK45 steps: the
 * record's Sigma slot (doubles 91..97) holds the drag column G_k in Sigma_k's place,
 *   G_k = d x_k+1 / d beta = A_k int Phi(tau)^-1 tf [0; a_D(x(tau)); 0] dtau,
 * the sensitivity of the interval's end state to a scale (1 + beta) on the drag acceleration a_D -- the fixed density's, or the
 * context's atmosphere's under MPCX_FLAG_ATMO -- over the same accepted nodes, by the same trapezoid and the same A_k as the other
 * columns; its mass row is 0.  A, B_kn, B_kp and xi of such a record are, to the bit, what the call without the bit writes, and the
 * steps are the same.  The solver cannot read such a record (it needs Sigma): mpcx_covariance_drag_batch does.  The bit without
 * MPCX_FLAG_DRAG, with MPCX_FLAG_UNIFORM_STEPS or with MPCX_FLAG_RK23: MPCX_E_BADARG with "discretize" in the message, nothing
 * enqueued.  The reference-layout discretize calls and the fused step ignore the bit; every other entry point treats it as the
 * unknown flag it is there. */
#define MPCX_FLAG_DRAG_COLUMN 64

/* normalised constants per satellite: reference constants.py:11-20 field order */
enum { MPCX_C_MU = 0, MPCX_C_R_E, MPCX_C_J2, MPCX_C_G0, MPCX_C_ISP, MPCX_C_S, MPCX_C_R0,
       MPCX_C_RHO, MPCX_NCONST };

/* packed per-interval stage record written by the discretizer and read by the solver:
 * [A 7x7 | B_kn 7x3 | B_kp 7x3 | Sigma 7 | xi 7], row-major blocks */
#define MPCX_STAGE_DOUBLES 105

typedef struct mpcx_ctx mpcx_ctx;

int mpcx_version(void);
/* one context per (device, host thread); calls on different contexts are thread-safe */
int mpcx_create(int device, mpcx_ctx **out);
void mpcx_destroy(mpcx_ctx *ctx);
const char *mpcx_last_error(const mpcx_ctx *ctx); /* ctx may be NULL: last create error */
int mpcx_synchronize(mpcx_ctx *ctx, void *stream);
/* The stream the HOST-POINTER entry points of this context work on (a context handle per (device, stream)).  A
 * context starts with a private non-blocking stream, so that contexts of different host threads overlap (one per device, or
 * several per device).  A process that drives the device through a stream of its own -- PyTorch's, say -- may hand that
 * stream in instead: the context's calls are then ordered with the rest of that stream's work.  stream: a hipStream_t, NULL
 * for the device's default stream, MPCX_STREAM_PRIVATE for a new private stream.  The old stream is drained first. */
#define MPCX_STREAM_PRIVATE ((void *)(intptr_t)-1)
int mpcx_set_stream(mpcx_ctx *ctx, void *stream);
/* The atmosphere of the world this context simulates, for the calls that carry MPCX_FLAG_ATMO: one closed form with four
 * coefficients atmo[MPCX_NATMO] = {c0, c1, c2, h_floor} in physical units,
 *   alt = |r R0| - R_EARTH  (metres; the altitude of Simulator.get_atmo_density, simulator.py:109, R_EARTH = 6.371e6)
 *   h = max(alt, h_floor),   rho(h) = exp(c0 + c1 ln h + c2 h)  kg/m^3,   d rho / d h = rho (c1 / h + c2) above the floor, 0 on it.
 * The Harris-Priester power fit a h^-b the reference keeps commented out (simulator.py:110: a = 8e26, b = 6.828) is
 * c0 = ln a, c1 = -b, c2 = 0; the exponential atmosphere rho_ref exp(-(h - h_ref) / H) is c0 = ln rho_ref + h_ref / H, c1 = 0,
 * c2 = -1 / H.  h_floor > 0 keeps the logarithm defined wherever a trial stage of an integrator lands.  The drag acceleration
 * uses rho / consts[s][MPCX_C_RHO] and the linearisation drho = (d rho / d h) consts[s][MPCX_C_R0] / consts[s][MPCX_C_RHO]:
 * the model is launch-wide, each satellite's units enter through its constants.  The coefficients are copied into the context
 * here and into the kernel arguments at every launch (no kernel reads the context; a later change does not reach work already
 * enqueued).  atmo = NULL clears them.  Non-finite coefficients or h_floor <= 0: MPCX_E_BADARG, the context keeps what it had. */
enum { MPCX_ATMO_C0 = 0, MPCX_ATMO_C1, MPCX_ATMO_C2, MPCX_ATMO_HFLOOR, MPCX_NATMO };
int mpcx_set_atmosphere(mpcx_ctx *ctx, const double *atmo);
/* Where a host-pointer call's time went, as data (the reference has no counterpart: its solve is a subprocess whose time
 * optimizer.py:603 does not look at).  mpcx_trace_enable(ctx, 1): every following host-pointer call on the context records, at
 * the price of four events and one polled marker per call,
 *   MPCX_TR_WALL          entry to return on the host, ms
 *   MPCX_TR_FIRST_MARKER  from entry until the stream has executed the call's FIRST packet (a bare marker, polled): time the
 *                         queue took to pick the call up -- before any work of this library ran
 *   MPCX_TR_HOST_STAGE    host copies into the staging pool + enqueueing of transfers and kernels
 *   MPCX_TR_HOST_WAIT     host blocked on the stream (events of the downloads, final synchronisation)
 *   MPCX_TR_HOST_COPYOUT  staging -> the caller's result arrays
 *   MPCX_TR_DEV_SPAN      the device's own time stamps: first marker -> last download done (includes any time the stream sat
 *                         waiting for the host to enqueue the next transfer)
 *   MPCX_TR_DEV_KERNELS   ... last upload done -> kernels done: the call's kernels alone, as the device ran them
 *   MPCX_TR_VALID         1 when the record belongs to a traced call
 * mpcx_last_call_trace copies the record of the context's last traced call (n <= MPCX_TRACE_N doubles).  The same marks are
 * printed to stderr for calls slower than MPCX_HOST_TRACE=<ms> (environment), with or without mpcx_trace_enable. */
enum { MPCX_TR_WALL = 0, MPCX_TR_FIRST_MARKER = 1, MPCX_TR_HOST_STAGE = 2, MPCX_TR_HOST_WAIT = 3, MPCX_TR_HOST_COPYOUT = 4,
       MPCX_TR_DEV_SPAN = 5, MPCX_TR_DEV_KERNELS = 6, MPCX_TR_VALID = 7, MPCX_TRACE_N = 8 };
int mpcx_trace_enable(mpcx_ctx *ctx, int on);
int mpcx_last_call_trace(const mpcx_ctx *ctx, double *out, int n);
/* Page-locked host memory for the arrays a caller hands to the host-pointer entry points again and again (the reference
 * keeps x_bar / u_bar / results in numpy arrays, optimizer.py:13-39, 192-217; a numpy array can live in such a buffer).
 * Arrays in page-locked memory are transferred by DMA straight from / to the caller's buffer; pageable ones go through the
 * context's own page-locked staging (an extra host copy each way). */
void *mpcx_host_alloc(mpcx_ctx *ctx, size_t bytes);
void mpcx_host_free(mpcx_ctx *ctx, void *p);

/*
 * Replaces Discretizer.discretize (linearize_discretize.py:334-390), i.e. get_matrices (:8-82)
 * for every interval of every satellite, including dPhi (:257-291), A_func (:119-183),
 * B_func (:186-215), xi_func (:218-236), Sigma_func (:239-254), u_FOH (:294-315) and the
 * RK45 integration the reference delegates to scipy (rtol 1e-3, atol 1e-6, max_step, automatic
 * first step), with f = Simulator.satellite_dynamics (simulator.py:116-161).
 *   xbar   [S][7][K]     reference trajectories         ubar [S][3][Ku]  reference thrust
 *   tf     [S]           reference final times          consts [S][MPCX_NCONST]
 *   A      [S][K-1][7][7]   Bp, Bn [S][K-1][7][3]   Sigma, xi [S][7][K-1]   (reference shapes,
 *   reference return order A, B_kp, B_kn, Sigma, xi)     status [S]
 */
int mpcx_discretize_batch(mpcx_ctx *ctx, int S, int K, int Ku, const double *xbar,
                          const double *ubar, const double *tf, const double *consts, int flags,
                          double max_step, double *A, double *Bp, double *Bn, double *Sigma,
                          double *xi, int32_t *status);
int mpcx_discretize_batch_dev(mpcx_ctx *ctx, int S, int K, int Ku, const double *xbar,
                              const double *ubar, const double *tf, const double *consts,
                              int flags, double max_step, double *A, double *Bp, double *Bn,
                              double *Sigma, double *xi, int32_t *status, void *stream);
/* same computation, output as packed stage records stage[S][K-1][MPCX_STAGE_DOUBLES] (the
 * layout the solver consumes; A/B never take the reference's five-array form) */
int mpcx_discretize_stages_dev(mpcx_ctx *ctx, int S, int K, int Ku, const double *xbar,
                               const double *ubar, const double *tf, const double *consts,
                               int flags, double max_step, double *stage, int32_t *status,
                               void *stream);

/* Options of the per-satellite solve: the keys of Optimizer.init_options (optimizer.py:178-188;
 * u_lim[1] -> u_max, r_lim -> r_min/r_max; r_des is per satellite; eps_vt is read only with
 * MPCX_SOLVE_LINEAR_VT: the reference as shipped enables the exact tangential constraint :577, which has no
 * tolerance) and the ipopt-level controls. */
typedef struct {
    double min_mass, u_max, r_min, r_max, eps_r, eps_vr, eps_vn, eps_vt, tf_max, w_nu, w_tr;
    double tol, acceptable_tol;
    int32_t max_iter, acceptable_iter, n_refine, flags;   /* flags: MPCX_SOLVE_* */
} mpcx_solve_opts;

/* By default the solver launches its per-satellite workgroups longest-first, ordered by the iteration counts of
 * the previous solve of the same batch size on this context (consecutive MPC steps pose similar problems; with a
 * few satellites per wave slot the launch ends when the slowest slot does).  Results never depend on the launch
 * order.  The counts are the library's own copy, written and read on the stream of the calls: consecutive solves on
 * one context must be enqueued on the same stream (or be ordered by the caller).  This flag keeps the plain index
 * order.  With it, solves of one context may be in flight on different streams at once: every launch has its own work
 * queue (up to 64 launches of a context in flight) and works in the caller's workspace; the regularisation record
 * (mpcx_solve_regularised) is then that of whichever solve wrote last. */
#define MPCX_SOLVE_INDEX_ORDER 1
/* Tangential velocity as the linearised pair max_tan_vel_rule / min_tan_vel_rule (optimizer.py:471-489,
 * |Vt_lin(x_K) - Vc_lin(r_K)| <= eps_vt), which the reference keeps commented out at :575-576, instead of the quartic
 * equality :492-517 it enables at :577.  Every constraint is then linear or convex quadratic and the objective strictly
 * convex in (x, u, tf): the minimiser is unique -- the variant the parity tests use to compare solvers exactly. */
#define MPCX_SOLVE_LINEAR_VT 2
/* The final time is not a variable: satellite s is solved with tf held at the value found in tf_out[s] ON ENTRY (its
 * range constraint optimizer.py:588 and its stationarity row drop out; the trust-region term w_tr (tf - tf_bar)^2 stays in
 * the objective as a constant).  ON EXIT tf_out[s] holds the satellite's term of the tf stationarity row,
 * g_s = 2 w_tr (tf - tf_bar) - sum_k Sigma_k . lambda_k = dV_s/dtf of its optimal value.  This is the inner problem of the
 * shared-tf mode: several satellites in one reference Optimizer share ONE tf (optimizer.py:287,311,322,336), and that NLP
 * separates given tf -- its KKT conditions are every inner problem's plus 1 + sum_s g_s(tf) = 0 (or tf on its bound),
 * a scalar equation the host solves (mpconstellation_amd/optimizer.py: Optimizer with shared tf).  Host-pointer entry
 * points read tf_out as an input too in this mode. */
#define MPCX_SOLVE_FIXED_TF 4

/* ONE final time for all S satellites of the call: the NLP of a reference Optimizer that holds several satellites
 * (optimizer.py:287: a single tf Var; its trust-region term :311,322 and the dynamics' Sigma_k tf :336 for every satellite,
 * the range constraint :588 once), solved as one problem -- one barrier parameter, one step length, one convergence test,
 * the tf row of every Newton system assembled across the satellites -- in a single cooperative launch with one workgroup per
 * satellite.  tf_out[s] is the same for every s (get_solved_tf ignores s, :199-203); status, iters, kkt are the launch's.
 * S is limited to the workgroups the device holds at once (2048 on MI355X); no ragged batches. */
#define MPCX_SOLVE_SHARED_TF 8

/* Batches of at most 1024 satellites (no more than one per SIMD of an MI355X) are solved by a kernel with TWO waves per
 * satellite that share the factorisation of every interior-point iteration.  Its results are bit for bit those of the
 * one-wave kernel larger batches use (both are compiled with -ffp-contract=on: the same expressions round alike): a
 * satellite's result does not depend on the size of the batch it is solved in.  This flag keeps the one-wave kernel for
 * small batches too (measurements, tests). */
#define MPCX_SOLVE_ONE_WAVE 16
/* Batches of at most one satellite per compute unit (256 on an MI355X) whose horizon's working set fits (K <= 30) are solved
 * with that working set -- iterate, direction, Newton and factor records, channel vectors: 134 KB at K = 30 -- held in the
 * compute unit's LDS instead of the global workspace (same kernel otherwise, same bits).  This flag keeps them on the
 * global-workspace kernel (measurements, tests). */
#define MPCX_SOLVE_NO_LDS 32
/* Time-parallel linear solve for small batches: the horizon is cut into four segments whose Riccati recursions and sweeps run
 * side by side, a workgroup of two waves per segment on its own compute unit, joined by a coarse 7 x 7 recursion over the cuts
 * (csrc/solve_tp.hip).  Honoured for batches of at most 128 satellites and row lengths K >= 24 (four
 * workgroups per satellite, all resident); other calls take the kernels they would take without the flag.  Same Newton
 * directions to ~1e-10 relative, the same iteration counts on 98-100 % of the problems, NOT the same bits as the other
 * kernels -- which is why it is a flag and not the default.  64 satellites: solve kernel 1.09 against 1.33 ms at 30 nodes, call 1.76
 * against 2.36 ms at 60.  The satellite's workgroups wait for each other (a cooperative launch, every wait with a
 * time limit that ends that satellite's solve with MPCX_ST_TIMEOUT): one time-parallel solve per device at a time -- a long
 * kernel of another stream or context that keeps some of a satellite's workgroups from becoming resident runs the limit out.
 * A batch the device cannot hold at once (more satellites than a quarter of its resident workgroups) takes the default kernels,
 * like a batch above 128. */
#define MPCX_SOLVE_TIME_PARALLEL 64
/* Test hook of the time-parallel kernel (tests/test_time_parallel_oracle_gpu.py): the workgroup of every satellite's first
 * segment leaves before its first command, so that the wait limit runs out -- every satellite must come back MPCX_ST_TIMEOUT with
 * defined results and the launch must end.  No effect without MPCX_SOLVE_TIME_PARALLEL. */
#define MPCX_SOLVE_TP_SELFTEST_DEAD (1 << 30)

void mpcx_default_solve_opts(mpcx_solve_opts *o);

/* Per-satellite problem options.  The eleven PROBLEM options of mpcx_solve_opts -- its first eleven doubles, in this order --
 * as a table popts [S][MPCX_NPOPT], row s for satellite s (satellite index: whatever order the launch takes the satellites in,
 * whichever half of a split update holds them).  A constellation whose satellites each live in their own units
 * (SatelliteScale per satellite) states a physical keep-out radius, maximum thrust or dry mass as a different normalised number
 * for every satellite; one call with a table replaces one call per distinct option set, and satellite s gets bit for bit what a
 * call with row s as its scalar options gives it.  The *_sat entry points below take the table directly after `opts`; the
 * solver controls (tol, acceptable_tol, max_iter, acceptable_iter, n_refine) and the flags stay those of `opts` for the whole
 * launch, and the table replaces all eleven problem options of `opts`.  A NULL table is the entry point without _sat: every
 * one of those is its _sat form with NULL.  Host-pointer variants take a host table, _dev variants a device table.
 * MPCX_SOLVE_SHARED_TF with a table is MPCX_E_BADARG (one tf cannot have per-satellite tf_max); MPCX_SOLVE_FIXED_TF is allowed.
 * A row whose constraint set is empty (r_min > r_max, tf_max <= 0, a terminal window outside r_max) gives that satellite alone
 * MPCX_ST_INFEASIBLE. */
enum { MPCX_PO_MIN_MASS = 0, MPCX_PO_U_MAX, MPCX_PO_R_MIN, MPCX_PO_R_MAX, MPCX_PO_EPS_R, MPCX_PO_EPS_VR, MPCX_PO_EPS_VN,
       MPCX_PO_EPS_VT, MPCX_PO_TF_MAX, MPCX_PO_W_NU, MPCX_PO_W_TR, MPCX_NPOPT };
/* Workspace of the _dev solves / fused steps.  It need not be initialised: a call's results do not depend on what the
 * workspace holds on entry -- any bit pattern, another call's leftovers (tests/test_stale_memory_gpu.py) -- and its contents
 * after the call are unspecified.  The plain queries are device-independent upper bounds (one slot per
 * satellite); the _ctx queries return what a launch on the context's device touches -- one slot per persistent workgroup,
 * min(S, workgroups resident at once: 2048 on MI355X), 0.44 GB instead of 1.8 GB at S = 8192, K = 30 -- and are enough. */
size_t mpcx_solve_workspace_bytes(int S, int K);
size_t mpcx_mpc_step_workspace_bytes(int S, int K);
size_t mpcx_solve_workspace_bytes_ctx(const mpcx_ctx *ctx, int S, int K);
size_t mpcx_mpc_step_workspace_bytes_ctx(const mpcx_ctx *ctx, int S, int K);

/*
 * Replaces Optimizer.get_constraint_terms (optimizer.py:80-170) + the NLP transcription and
 * ipopt solve of Optimizer.solve_OPT (optimizer.py:254-613), one independent problem (own tf)
 * per satellite, given already discretised dynamics.
 *   host variant: A [S][K-1][7][7], Bp, Bn [S][K-1][7][3], Sigma, xi [S][7][K-1] in the reference's
 *   shapes; device variant: packed stage records stage[S][K-1][MPCX_STAGE_DOUBLES].
 *   xbar [S][7][K], ubar [S][3][K], tf [S], consts [S][MPCX_NCONST], r_des [S]
 * Results replace get_solved_trajectory / get_solved_u / get_solved_nu / get_solved_tf
 * (optimizer.py:192-217): X [S][7][K], U [S][3][K], NU [S][7][K], tf_out [S];
 * status [S] (MPCX_ST_*), iters [S], kkt [S] = final scaled optimality error (ipopt's E_0).
 */
int mpcx_solve_batch(mpcx_ctx *ctx, int S, int K, const double *A, const double *Bp, const double *Bn,
                     const double *Sigma, const double *xi, const double *xbar, const double *ubar,
                     const double *tf, const double *consts, const double *r_des,
                     const mpcx_solve_opts *opts, double *X, double *U, double *NU, double *tf_out,
                     int32_t *status, int32_t *iters, double *kkt);
int mpcx_solve_batch_dev(mpcx_ctx *ctx, int S, int K, const double *stage, const double *xbar,
                         const double *ubar, const double *tf, const double *consts,
                         const double *r_des, const mpcx_solve_opts *opts, double *X, double *U,
                         double *NU, double *tf_out, int32_t *status, int32_t *iters, double *kkt,
                         void *workspace, void *stream);
/* ... with per-satellite problem options popts [S][MPCX_NPOPT] (MPCX_PO_*; NULL: the calls above) */
int mpcx_solve_batch_sat(mpcx_ctx *ctx, int S, int K, const double *A, const double *Bp, const double *Bn,
                         const double *Sigma, const double *xi, const double *xbar, const double *ubar,
                         const double *tf, const double *consts, const double *r_des,
                         const mpcx_solve_opts *opts, const double *popts, double *X, double *U, double *NU, double *tf_out,
                         int32_t *status, int32_t *iters, double *kkt);

/* Per-satellite regularisation record of the LAST solve (or fused step) on this context, out [S][2] int32: the number of
 * interior-point iterations whose Newton system needed a Hessian regularisation delta_w > 0 (ipopt's inertia correction:
 * its iteration log prints the same quantity, lg(rg), which optimizer.py:603 shows with tee=verbose), and the index of the
 * first such iteration (-1: none).  S must be that solve's batch size.  The _dev variant copies on `stream` (the stream of
 * the solve) into device memory; the host variant returns when `out` is filled. */
int mpcx_solve_regularised(mpcx_ctx *ctx, int S, int32_t *out);
int mpcx_solve_regularised_dev(mpcx_ctx *ctx, int S, int32_t *out, void *stream);

/*
 * Replaces Optimizer.get_constraint_terms (optimizer.py:80-170) as the solver consumes it: what the device builds for
 * every satellite before its first iteration, returned instead of used.  Terminal inequality rows a_j . x_K <= b_j,
 *   aT [S][8][7], bT [S][8]:  0: -r_hat.r_K <= -(r_des - eps_r)          (optimizer.py:398-402)
 *                             1, 2: +-(Vr linearised) <= eps_vr           (:406-416, 432-433)
 *                             3, 4: +-(Vn linearised) <= eps_vn           (:436-446, 466-467; Dv_h_hat in its precedence form :122)
 *                             5: -m_K <= -min_mass                        (:351-352, 363)
 *                             6, 7: +-(Vt - Vc linearised) <= eps_vt      (:471-489; zero rows without MPCX_SOLVE_LINEAR_VT)
 * every b relaxed by 1e-8 max(1, |b|) (ipopt's bound_relax_factor), and
 *   scalars [S][MPCX_NTERM_SCALARS]: relaxed u_max^2 (:379-381), r_max^2 (:393-395), -r_min (:384-391), (r_des+eps_r)^2
 *   (:403), the tf range 0 / tf_max (:588), vt_des = sqrt(mu / r_des) (:492-517), and the structural violation (> 0: the
 *   constraint set is empty, MPCX_ST_INFEASIBLE).
 * xbar [S][7][K], consts [S][MPCX_NCONST], r_des [S].
 */
#define MPCX_NTERM_SCALARS 8
int mpcx_constraint_terms(mpcx_ctx *ctx, int S, int K, const double *xbar, const double *consts,
                          const double *r_des, const mpcx_solve_opts *opts, double *aT, double *bT, double *scalars);
int mpcx_constraint_terms_dev(mpcx_ctx *ctx, int S, int K, const double *xbar, const double *consts,
                              const double *r_des, const mpcx_solve_opts *opts, double *aT, double *bT,
                              double *scalars, void *stream);
/* ... every satellite's terms under its own row of popts [S][MPCX_NPOPT] (NULL: the calls above) */
int mpcx_constraint_terms_sat(mpcx_ctx *ctx, int S, int K, const double *xbar, const double *consts,
                              const double *r_des, const mpcx_solve_opts *opts, const double *popts, double *aT, double *bT,
                              double *scalars);
int mpcx_constraint_terms_sat_dev(mpcx_ctx *ctx, int S, int K, const double *xbar, const double *consts,
                                  const double *r_des, const mpcx_solve_opts *opts, const double *popts, double *aT, double *bT,
                                  double *scalars, void *stream);

/*
 * One satellite-MPC-step = Optimizer.solve_OPT as the reference runs it (optimizer.py:243-251 calls
 * discretize, then :254-603): discretize -> constraint terms -> solve, fused on the device; the
 * stage records never take the reference's five-array form and never leave HBM.
 */
int mpcx_mpc_step_batch(mpcx_ctx *ctx, int S, int K, const double *xbar, const double *ubar,
                        const double *tf, const double *consts, const double *r_des, int flags,
                        double max_step, const mpcx_solve_opts *opts, double *X, double *U, double *NU,
                        double *tf_out, int32_t *status, int32_t *iters, double *kkt);
int mpcx_mpc_step_batch_dev(mpcx_ctx *ctx, int S, int K, const double *xbar, const double *ubar,
                            const double *tf, const double *consts, const double *r_des, int flags,
                            double max_step, const mpcx_solve_opts *opts, double *X, double *U,
                            double *NU, double *tf_out, int32_t *status, int32_t *iters, double *kkt,
                            void *workspace, void *stream);

/* thrust laws of the reference's controllers (control.py) */
#define MPCX_CTRL_ZERO 0        /* Controller.get_u_func            control.py:20-29  */
#define MPCX_CTRL_CONSTANT 1    /* ConstantThrustController          control.py:37-53  ctrl_vec [S][3]      */
#define MPCX_CTRL_TANGENTIAL 2  /* ConstantTangentialThrustController control.py:55-84 ctrl_vec [S] magnitude */
#define MPCX_CTRL_SEQUENCE 3    /* SequenceController (FOH playback) control.py:86-143 ctrl_vec [S][3][Ku], end_tau [S] */

/*
 * Replaces Simulator.get_trajectory_ODE (simulator.py:164-189) for S satellites: scipy
 * solve_ivp(RK45, rtol 1e-3, atol 1e-6, max_step, t_eval=linspace(0,1,n_eval)) of
 * Simulator.satellite_dynamics (simulator.py:116-161, flags = MPCX_FLAG_DRAG|MPCX_FLAG_J2[|MPCX_FLAG_ATMO]) under a
 * thrust law u(y, tau).  y0 [S][7] normalised states, y_out [S][7][n_eval] (= sol.y per satellite).
 */
int mpcx_propagate_batch(mpcx_ctx *ctx, int S, int n_eval, const double *y0, const double *tf,
                         const double *consts, int flags, int ctrl_kind, const double *ctrl_vec, int Ku,
                         const double *end_tau, double max_step, double *y_out, int32_t *status,
                         int32_t *nsteps);
int mpcx_propagate_batch_dev(mpcx_ctx *ctx, int S, int n_eval, const double *y0, const double *tf,
                             const double *consts, int flags, int ctrl_kind, const double *ctrl_vec,
                             int Ku, const double *end_tau, double max_step, double *y_out,
                             int32_t *status, int32_t *nsteps, void *stream);

/*
 * Ragged batches.  The reference re-samples every SCP re-rollout at int(base_res * tf_u) nodes (control.py:227 ->
 * simulator.py:38), a different count for every satellite of a constellation: the next discretize / solve then has K_s
 * nodes for satellite s.  The *_ragged entry points take one launch of satellites with different counts: arrays keep the
 * rectangular shapes of the plain entry points with K (n_eval, Ku) the ROW LENGTH, and satellite s uses the first Ks[s]
 * (n_evals[s], Kus[s]) columns of its rows; np.linspace(0, 1, Ks[s]) is its node grid.  Input columns past a satellite's
 * count are never read: they may hold anything.  Result columns past a satellite's count come back zero (stage records past
 * its last interval are unspecified).  In the _dev variants: the solves and fused steps write those zeros themselves, into
 * every row of X, U and NU -- except for a satellite that comes back MPCX_ST_BADK or MPCX_ST_INFEASIBLE, whose reference rows
 * are handed back whole, the columns past its count as they came in; mpcx_resample_sequence_dev writes them too; the
 * propagate _dev variants leave the columns of y_out / u_out past n_evals[s] untouched (the host variants clear them).
 * A count outside the accepted range gives that satellite MPCX_ST_BADK and leaves the others alone.  A NULL count array means "all K": the plain entry points are
 * these with NULL.  Count arrays are int32; device pointers in the _dev variants.
 */
int mpcx_discretize_stages_ragged_dev(mpcx_ctx *ctx, int S, int K, const int32_t *Ks, int Ku, const int32_t *Kus,
                                      const double *xbar, const double *ubar, const double *tf,
                                      const double *consts, int flags, double max_step, double *stage,
                                      int32_t *status, void *stream);
int mpcx_solve_batch_ragged_dev(mpcx_ctx *ctx, int S, int K, const int32_t *Ks, const double *stage, const double *xbar,
                                const double *ubar, const double *tf, const double *consts,
                                const double *r_des, const mpcx_solve_opts *opts, double *X, double *U,
                                double *NU, double *tf_out, int32_t *status, int32_t *iters, double *kkt,
                                void *workspace, void *stream);
/* the fused step: thrust tables have as many columns as the satellite has nodes (Kus = Ks) */
int mpcx_mpc_step_batch_ragged(mpcx_ctx *ctx, int S, int K, const int32_t *Ks, const double *xbar, const double *ubar,
                               const double *tf, const double *consts, const double *r_des, int flags,
                               double max_step, const mpcx_solve_opts *opts, double *X, double *U, double *NU,
                               double *tf_out, int32_t *status, int32_t *iters, double *kkt);
int mpcx_mpc_step_batch_ragged_dev(mpcx_ctx *ctx, int S, int K, const int32_t *Ks, const double *xbar, const double *ubar,
                                   const double *tf, const double *consts, const double *r_des, int flags,
                                   double max_step, const mpcx_solve_opts *opts, double *X, double *U,
                                   double *NU, double *tf_out, int32_t *status, int32_t *iters, double *kkt,
                                   void *workspace, void *stream);
/* the ragged solve and fused step with per-satellite problem options popts [S][MPCX_NPOPT] (MPCX_PO_*; NULL: the calls above) */
int mpcx_solve_batch_ragged_sat_dev(mpcx_ctx *ctx, int S, int K, const int32_t *Ks, const double *stage, const double *xbar,
                                    const double *ubar, const double *tf, const double *consts,
                                    const double *r_des, const mpcx_solve_opts *opts, const double *popts, double *X, double *U,
                                    double *NU, double *tf_out, int32_t *status, int32_t *iters, double *kkt,
                                    void *workspace, void *stream);
int mpcx_mpc_step_batch_ragged_sat(mpcx_ctx *ctx, int S, int K, const int32_t *Ks, const double *xbar, const double *ubar,
                                   const double *tf, const double *consts, const double *r_des, int flags,
                                   double max_step, const mpcx_solve_opts *opts, const double *popts, double *X, double *U,
                                   double *NU, double *tf_out, int32_t *status, int32_t *iters, double *kkt);
int mpcx_mpc_step_batch_ragged_sat_dev(mpcx_ctx *ctx, int S, int K, const int32_t *Ks, const double *xbar, const double *ubar,
                                       const double *tf, const double *consts, const double *r_des, int flags,
                                       double max_step, const mpcx_solve_opts *opts, const double *popts, double *X, double *U,
                                       double *NU, double *tf_out, int32_t *status, int32_t *iters, double *kkt,
                                       void *workspace, void *stream);
/* Simulator.get_trajectory_ODE with t_eval = linspace(0, 1, n_evals[s]) per satellite (simulator.py:38,185-187) and, for
 * MPCX_CTRL_SEQUENCE, thrust tables of Kus[s] columns */
int mpcx_propagate_batch_ragged(mpcx_ctx *ctx, int S, int n_eval, const int32_t *n_evals, const double *y0,
                                const double *tf, const double *consts, int flags, int ctrl_kind,
                                const double *ctrl_vec, int Ku, const int32_t *Kus, const double *end_tau,
                                double max_step, double *y_out, int32_t *status, int32_t *nsteps);
int mpcx_propagate_batch_ragged_dev(mpcx_ctx *ctx, int S, int n_eval, const int32_t *n_evals, const double *y0,
                                    const double *tf, const double *consts, int flags, int ctrl_kind,
                                    const double *ctrl_vec, int Ku, const int32_t *Kus, const double *end_tau,
                                    double max_step, double *y_out, int32_t *status, int32_t *nsteps, void *stream);
/*
 * The same rollout that also returns Discretizer.extract_uk (linearize_discretize.py:393-411) of its controller: u_out
 * [S][3][n_eval] = u_func(x_k, t_k) at every output point (control.py:66-84 for the tangential law, :104-142 for a
 * sequence, the constant vector, zeros) -- the reference thrust u_bar that OptimalController.update (control.py:187,222)
 * derives from the trajectory it has just computed.  u_out may be NULL (then it is mpcx_propagate_batch_ragged).
 */
int mpcx_propagate_thrust_batch_ragged(mpcx_ctx *ctx, int S, int n_eval, const int32_t *n_evals, const double *y0,
                                       const double *tf, const double *consts, int flags, int ctrl_kind,
                                       const double *ctrl_vec, int Ku, const int32_t *Kus, const double *end_tau,
                                       double max_step, double *y_out, double *u_out, int32_t *status, int32_t *nsteps);
int mpcx_propagate_thrust_batch_ragged_dev(mpcx_ctx *ctx, int S, int n_eval, const int32_t *n_evals, const double *y0,
                                           const double *tf, const double *consts, int flags, int ctrl_kind,
                                           const double *ctrl_vec, int Ku, const int32_t *Kus, const double *end_tau,
                                           double max_step, double *y_out, double *u_out, int32_t *status, int32_t *nsteps,
                                           void *stream);
/*
 * One SCP iteration of OptimalController.update (control.py:183-227) for S satellites in one call: the nonlinear rollout from
 * y0 [S][7] over tf [S] under the given thrust law (arguments as mpcx_propagate_batch_ragged), sampled at K nodes (Ks[s] of
 * them in a ragged batch) -- x_bar; the law at those nodes -- u_bar (extract_uk); the discretisation about (x_bar, u_bar,
 * tf) and the solve (arguments and results as mpcx_mpc_step_batch_ragged).  x_bar and u_bar stay on the device; they are
 * returned only when xbar_out [S][7][K] / ubar_out [S][3][K] are not NULL.  prop_status [S]: the rollout's MPCX_ST_* codes.
 */
int mpcx_scp_iteration_batch_ragged(mpcx_ctx *ctx, int S, int K, const int32_t *Ks, const double *y0, const double *tf,
                                    const double *consts, const double *r_des, int prop_flags, int ctrl_kind,
                                    const double *ctrl_vec, int Ku, const int32_t *Kus, const double *end_tau,
                                    double prop_max_step, int disc_flags, double disc_max_step, const mpcx_solve_opts *opts,
                                    double *xbar_out, double *ubar_out, double *X, double *U, double *NU, double *tf_out,
                                    int32_t *status, int32_t *iters, double *kkt, int32_t *prop_status);
/* ... with per-satellite problem options popts [S][MPCX_NPOPT] (MPCX_PO_*; NULL: the call above) */
int mpcx_scp_iteration_batch_ragged_sat(mpcx_ctx *ctx, int S, int K, const int32_t *Ks, const double *y0, const double *tf,
                                        const double *consts, const double *r_des, int prop_flags, int ctrl_kind,
                                        const double *ctrl_vec, int Ku, const int32_t *Kus, const double *end_tau,
                                        double prop_max_step, int disc_flags, double disc_max_step, const mpcx_solve_opts *opts,
                                        const double *popts, double *xbar_out, double *ubar_out, double *X, double *U, double *NU,
                                        double *tf_out, int32_t *status, int32_t *iters, double *kkt, int32_t *prop_status);
/*
 * OptimalController.update (control.py:170-235) for S satellites in ONE call -- and, optionally, the segment flight of
 * Simulator.run_segment (simulator.py:58-65) that follows it -- with everything between the first input and the last result
 * resident in HBM: the reference rollout from y0 [S][7] over tf0 [S] (the horizon) under ConstantTangentialThrustController
 * (ref_thrust; control.py:178-180) sampled at K = int(base_res * horizon) nodes, then n_scp x [ extract_uk, discretise, solve ]
 * (:183-213) with, between two iterations, the nonlinear re-rollout under SequenceController(u_opt, tf_u, tf_u) sampled at
 * int(base_res * tf_u) nodes per satellite (:217-227, simulator.py:38: the node counts are computed on the device and the
 * next iteration is a ragged launch; the plan's thrust is consumed in place as the rollout's table).
 * Results: the last iteration's plan X [S][7][K], U [S][3][K], NU [S][7][K] (rows of length K, Ks_out[s] columns in use, zeros
 * behind them), tf_out [S] = tf_u, Ks_out [S]; status, iters [n_scp][S]: every iteration's solver outcome; kkt [S]: the last
 * iteration's; prop_status [S]: the first failure among the rollouts (MPCX_ST_*).
 * disc_flags: the discretisation's flags (MPCX_FLAG_DRAG, MPCX_FLAG_J2, ...); with MPCX_FLAG_PLAN_ROLLOUTS the rollouts of the
 * plan use its MPCX_FLAG_DRAG | MPCX_FLAG_J2 | MPCX_FLAG_ATMO as well.
 * Segment flight (y_sim != NULL): from y0 over sim_tf under the truth model sim_flags (MPCX_FLAG_DRAG | MPCX_FLAG_J2 | MPCX_FLAG_ATMO) with
 * SequenceController(u_opt, tf_u, tf_sim = sim_interval) (end_tau = tf_u / sim_interval, control.py:102,217),
 * y_sim [S][7][sim_n_eval] = sol.y at linspace(0, 1, sim_n_eval), sim_status [S].
 * Environment (measurement switch, read per call): MPCX_UPDATE_SPLIT=1 runs a batch of 2048 or more satellites as two chains --
 * its halves, each on its own stream, so that one half's rollouts run under the other half's solve -- and =2 also delays the
 * second chain to the first's first solve; same bits either way; measured no faster than one chain, hence
 * not the default.
 */
int mpcx_mpc_update_batch(mpcx_ctx *ctx, int S, int K, int n_scp, double base_res, const double *y0, const double *tf0,
                          const double *consts, const double *r_des, double ref_thrust, double prop_max_step, int disc_flags,
                          double disc_max_step, const mpcx_solve_opts *opts, double *X, double *U, double *NU, double *tf_out,
                          int32_t *Ks_out, int32_t *status, int32_t *iters, double *kkt, int32_t *prop_status, double sim_tf,
                          double sim_interval, int sim_n_eval, int sim_flags, double sim_max_step, double *y_sim,
                          int32_t *sim_status);
/* ... with per-satellite problem options popts [S][MPCX_NPOPT] (MPCX_PO_*; NULL: the call above): every SCP iteration of the
 * update solves satellite s under row s, in either chain of a split update */
int mpcx_mpc_update_batch_sat(mpcx_ctx *ctx, int S, int K, int n_scp, double base_res, const double *y0, const double *tf0,
                              const double *consts, const double *r_des, double ref_thrust, double prop_max_step, int disc_flags,
                              double disc_max_step, const mpcx_solve_opts *opts, const double *popts, double *X, double *U,
                              double *NU, double *tf_out, int32_t *Ks_out, int32_t *status, int32_t *iters, double *kkt,
                              int32_t *prop_status, double sim_tf, double sim_interval, int sim_n_eval, int sim_flags,
                              double sim_max_step, double *y_sim, int32_t *sim_status);
/*
 * Replaces Discretizer.extract_uk (linearize_discretize.py:393-411) for a SequenceController played over its own horizon
 * (control.py:217-221, tf_sim = tf_u: end_tau = 1): the first-order hold (control.py:104-126) of table u [S][3][Ku]
 * (Kus[s] columns in use) at the nodes linspace(0, 1, ns[s]) -> u_out [S][3][n], the reference thrust of the next SCP
 * iteration.  status [S]: MPCX_ST_FOH / MPCX_ST_BADK.
 */
int mpcx_resample_sequence_dev(mpcx_ctx *ctx, int S, int Ku, const int32_t *Kus, const double *u, int n,
                               const int32_t *ns, double *u_out, int32_t *status, void *stream);

/*
 * Conjunction screening: the constellation on one clock, and the closest approach of every pair on it.  The reference flies
 * and plans every satellite in its own units and on its own clock and never looks at two satellites at once (simulator.py:68,87
 * leaves "scale the tfs so satellites orbit for the same time?" open).
 *
 * mpcx_ephemeris_batch: trajectories as the library returns them -- Y [S][7][n] normalised states (rows of length n, ns[s] nodes
 * in use; ns = NULL: all n; the ragged convention above) -- resampled at M >= 2 common instants linspace(T0, T1, M) (seconds; the
 * last instant is exactly T1) in physical units:
 *   units [S][2]   each satellite's length unit (m) and time unit (s); its speed unit is their quotient
 *   span  [S][2]   physical times (s) of the satellite's first and last node; the nodes are uniform in between
 *   eph   [S][6][M]   position (m) and velocity (m/s): cubic Hermite in physical time on the node positions and velocities (the
 *                     state carries the velocity, so the interpolant is C1; error h_n^4 / 384 max |p''''| for node spacing h_n)
 * An instant outside [span[s][0], span[s][1]] gives NaN in all six rows.  status [S]: ns[s] outside 2..n or span[s][1] <=
 * span[s][0] gives all NaN and MPCX_ST_BADK.  M < 2, S < 1, n < 1, T1 <= T0: MPCX_E_BADARG, nothing enqueued.
 *
 * mpcx_conjunction_screen: for the rows i = row0 .. row0 + nrows - 1 (a block of rows per device: every device is given the whole
 * eph; row0 = 0, nrows = S for all) against every column j != i, over every grid interval [t_m, t_m+1] (h = (T1 - T0) / (M - 1)),
 * skipping an interval where either satellite has a NaN among the six values of either end.  With lo = min(i, j), hi = max(i, j),
 * d = p_hi - p_lo and w = v_hi - v_lo at the two ends (so both orderings of a pair get the same bits):
 *   chord  D = d1 - d0,  s* = clamp(-d0 . D / |D|^2, 0, 1)  (0 when |D|^2 is zero or not finite);
 *   if 0 < s* < 1: three Newton steps on g(s) = d(s) . d'(s), d(s) the cubic Hermite of (d0, h w0, d1, h w1), g' = |d'|^2 + d . d'',
 *   a step skipped where g' <= 0, s clamped to [0, 1] after every step;
 *   the interval's distance is min(|d0|, |d1|, |d(s)|), its time that of the smallest (t_m, t_m+1, t_m + s h; of equal ones the
 *   first in this order).  Distances are compared as their squares.
 * Per row: dmin [nrows] (m), partner [nrows] (-1: none), tca [nrows] (s) -- the smallest distance, of equal ones the smaller j,
 * then the earlier interval; a row with no valid interval against anybody gets +inf, -1, NaN.
 * threshold > 0: every pair i < j (i among the rows) whose minimum over all intervals is <= threshold is appended to
 * pairs [max_pairs][4] = (i, j, distance, time), in no particular order; *n_pairs is the number of such pairs even when it
 * exceeds max_pairs (the list then holds some max_pairs of them).  threshold <= 0: no list, *n_pairs = 0 (n_pairs may be NULL).
 * M < 2, S < 1, T1 <= T0, max_pairs < 0, rows outside 0 .. S-1: MPCX_E_BADARG, nothing enqueued.
 * The host variant takes eph in host memory; the _dev variant takes device pointers throughout (n_pairs too) and a workspace of
 * mpcx_conjunction_workspace_bytes(S, M) bytes (the instant-major copy of eph and the partial minima; contents unspecified on
 * entry and exit).  Results do not depend on the block of rows a row is computed in.
 *
 * mpcx_conjunction_screen_traj: both steps in one call, from trajectories (host pointers) to results; eph stays in HBM.
 * status [S] (may be NULL): the ephemeris'.  Same bits as the two calls.
 */
int mpcx_ephemeris_batch(mpcx_ctx *ctx, int S, int n, const int32_t *ns, const double *Y, const double *units,
                         const double *span, int M, double T0, double T1, double *eph, int32_t *status);
int mpcx_ephemeris_batch_dev(mpcx_ctx *ctx, int S, int n, const int32_t *ns, const double *Y, const double *units,
                             const double *span, int M, double T0, double T1, double *eph, int32_t *status, void *stream);
size_t mpcx_conjunction_workspace_bytes(int S, int M);
int mpcx_conjunction_screen(mpcx_ctx *ctx, int S, int M, const double *eph, double T0, double T1, int row0, int nrows,
                            double threshold, int max_pairs, double *dmin, int32_t *partner, double *tca, double *pairs,
                            int64_t *n_pairs);
int mpcx_conjunction_screen_dev(mpcx_ctx *ctx, int S, int M, const double *eph, double T0, double T1, int row0, int nrows,
                                double threshold, int max_pairs, double *dmin, int32_t *partner, double *tca, double *pairs,
                                int64_t *n_pairs, void *workspace, void *stream);
int mpcx_conjunction_screen_traj(mpcx_ctx *ctx, int S, int n, const int32_t *ns, const double *Y, const double *units,
                                 const double *span, int M, double T0, double T1, int row0, int nrows, double threshold,
                                 int max_pairs, double *dmin, int32_t *partner, double *tca, double *pairs, int64_t *n_pairs,
                                 int32_t *status);

/*
 * Conjunction screening against a catalogue of foreign objects: rows are the constellation's satellites (eph [S][6][M]), columns
 * the objects of a catalogue (cat [D][6][M]: debris, other operators' satellites), both on the same grid linspace(T0, T1, M) -- two
 * mpcx_ephemeris_batch calls with the same M, T0, T1.  The rectangle S x D is computed, not the square of the union.
 *
 * mpcx_conjunction_cross_screen: for the rows i = row0 .. row0 + nrows - 1 against every object j = 0 .. D-1, over every grid
 * interval, skipping an interval where either of the two has a NaN among the six values of either end.  d = p_cat - p_sat and
 * w = v_cat - v_sat at the two ends, then the chord, the Newton steps and the interval's distance and time exactly as in
 * mpcx_conjunction_screen: the pair (i, j) gets the bits that screen gives the pair (i, S + j) of the union [eph; cat].
 * Per row: dmin [nrows] (m), partner [nrows] (an index into the CATALOGUE; -1: none), tca [nrows] (s) -- the smallest distance, of
 * equal ones the smaller j, then the earlier interval; a row with no valid interval against any object gets +inf, -1, NaN; an
 * object that is never on the grid is never a partner.
 * threshold > 0: every pair (i, j), i among the rows, whose minimum over all intervals is <= threshold is appended once to
 * pairs [max_pairs][4] = (i, j, distance, time), in no particular order; *n_pairs is the number of such pairs even when it
 * exceeds max_pairs.  threshold <= 0: no list, *n_pairs = 0 (n_pairs may be NULL).
 * M < 2, S < 1, D < 1, T1 <= T0, max_pairs < 0, rows outside 0 .. S-1: MPCX_E_BADARG, nothing enqueued.
 * The host variant takes eph and cat in host memory; the _dev variant takes device pointers throughout (n_pairs too) and a
 * workspace of mpcx_conjunction_cross_workspace_bytes(S, D, M) bytes (0 for S < 1, D < 1 or M < 2; the instant-major copies and
 * the partial minima; contents unspecified on entry and exit).  Results do not depend on the block of rows a row is computed in.
 *
 * mpcx_conjunction_cross_screen_traj: everything in one call, from trajectories (host pointers; the constellation's n, ns, Y, units,
 * span and the catalogue's own cat_n, cat_ns, cat_Y, cat_units, cat_span, as mpcx_ephemeris_batch takes them) to results; neither
 * ephemeris leaves HBM.  status [S], cat_status [D] (each may be NULL): the two ephemerides'.  Same bits as the three calls.
 */
size_t mpcx_conjunction_cross_workspace_bytes(int S, int D, int M);
int mpcx_conjunction_cross_screen(mpcx_ctx *ctx, int S, int D, int M, const double *eph, const double *cat, double T0, double T1,
                                  int row0, int nrows, double threshold, int max_pairs, double *dmin, int32_t *partner,
                                  double *tca, double *pairs, int64_t *n_pairs);
int mpcx_conjunction_cross_screen_dev(mpcx_ctx *ctx, int S, int D, int M, const double *eph, const double *cat, double T0,
                                      double T1, int row0, int nrows, double threshold, int max_pairs, double *dmin,
                                      int32_t *partner, double *tca, double *pairs, int64_t *n_pairs, void *workspace,
                                      void *stream);
int mpcx_conjunction_cross_screen_traj(mpcx_ctx *ctx, int S, int n, const int32_t *ns, const double *Y, const double *units,
                                       const double *span, int D, int cat_n, const int32_t *cat_ns, const double *cat_Y,
                                       const double *cat_units, const double *cat_span, int M, double T0, double T1, int row0,
                                       int nrows, double threshold, int max_pairs, double *dmin, int32_t *partner, double *tca,
                                       double *pairs, int64_t *n_pairs, int32_t *status, int32_t *cat_status);

/*
 * The closest approach of LISTED pairs: what the two screens compute for a pair, for the n pairs of a list alone -- n x M work
 * where a screen does S^2 x M or S x D x M.  A list that a screen made is looked at again after something changed the
 * trajectories (a manoeuvre flown, an orbit update of a few objects) without screening everybody against everybody once more.
 *
 * mpcx_conjunction_pairs: pairs [n][4], rows (i, j, -, -) as the screens list them; only columns 0 and 1 are read.  eph [S][6][M]
 * and, with D > 0, cat [D][6][M] on the grid linspace(T0, T1, M), as the screens take them.  D > 0: i indexes eph and j the
 * catalogue, d = p_cat - p_sat (mpcx_conjunction_cross_screen's pair).  D = 0 (cat NULL): i and j both index eph, in either order,
 * d = p_hi - p_lo (mpcx_conjunction_screen's pair; (i, j) and (j, i) get the same bits).  Per pair every grid interval is treated
 * exactly as mpcx_conjunction_screen describes, with the same skipping of intervals that have a NaN among the six values of an
 * end, and the pair's minimum is the smallest squared distance, of equal ones the earliest interval.
 *   out [n][4] = (i, j, distance in m, time in s) in list order, i and j as given; +inf and NaN for a pair without a valid interval.
 *   status [n]: MPCX_ST_OK; MPCX_ST_BADK for an index that is not a whole number inside its side, or i == j with D = 0 -- distance
 *   and time of that row are NaN and the other rows are not affected.
 * The distance and time of a pair are, bit for bit, those the screens list for it on the same eph, cat, M, T0, T1 (the same source
 * expressions, compiled with -ffp-contract=on; a minimum under a total order, so the result does not depend on how the intervals
 * are dealt out to lanes).  n < 1, S < 1, D < 0, M < 2, T1 <= T0, a missing array, cat given with D = 0 or missing with D > 0:
 * MPCX_E_BADARG, nothing enqueued.  The host variant takes host pointers; the _dev variant device pointers throughout, no
 * workspace, and enqueues one kernel on `stream`.
 *
 * mpcx_conjunction_pairs_traj: from trajectories, as mpcx_conjunction_screen_traj (D = 0; the cat_ arguments NULL / 0) and
 * mpcx_conjunction_cross_screen_traj (D > 0) take them; the ephemerides never leave HBM.  eph_status [S], cat_status [D]: the two
 * ephemerides' statuses (host variant: each may be NULL; cat_status is not written with D = 0).  Same bits as mpcx_ephemeris_batch
 * followed by mpcx_conjunction_pairs.  The _dev variant takes device pointers throughout (eph_status required, cat_status
 * required with D > 0) and a workspace of mpcx_conjunction_pairs_workspace_bytes(S, D, M) bytes (the ephemerides; 0 for S < 1,
 * D < 0 or M < 2; contents unspecified on entry and exit).
 */
size_t mpcx_conjunction_pairs_workspace_bytes(int S, int D, int M);
int mpcx_conjunction_pairs(mpcx_ctx *ctx, int n, const double *pairs, int S, int D, int M, const double *eph, const double *cat,
                           double T0, double T1, double *out, int32_t *status);
int mpcx_conjunction_pairs_dev(mpcx_ctx *ctx, int n, const double *pairs, int S, int D, int M, const double *eph, const double *cat,
                               double T0, double T1, double *out, int32_t *status, void *stream);
int mpcx_conjunction_pairs_traj(mpcx_ctx *ctx, int n, const double *pairs, int S, int nn, const int32_t *ns, const double *Y,
                                const double *units, const double *span, int D, int cat_n, const int32_t *cat_ns,
                                const double *cat_Y, const double *cat_units, const double *cat_span, int M, double T0, double T1,
                                double *out, int32_t *status, int32_t *eph_status, int32_t *cat_status);
int mpcx_conjunction_pairs_traj_dev(mpcx_ctx *ctx, int n, const double *pairs, int S, int nn, const int32_t *ns, const double *Y,
                                    const double *units, const double *span, int D, int cat_n, const int32_t *cat_ns,
                                    const double *cat_Y, const double *cat_units, const double *cat_span, int M, double T0,
                                    double T1, double *out, int32_t *status, int32_t *eph_status, int32_t *cat_status,
                                    void *workspace, void *stream);

/*
 * EVERY close approach of listed pairs.  mpcx_conjunction_pairs gives a pair's global minimum over the grid, which is all there is
 * in a window shorter than an orbit; over several revolutions two objects on crossing orbits come close about twice per
 * revolution, and each of those encounters has its own probability and wants its own look at a manoeuvre.  These calls return
 * them all, below a threshold, as rows (i, j, distance, time) -- the form every call that takes a pairs list takes, each row on
 * its own with the row's time as the encounter.
 *
 * The definition.  For a pair and the grid intervals m = 0 .. M-2 let (q_m, t_m) be the squared distance and the time that
 * mpcx_conjunction_screen describes for interval m ALONE, with the operands of mpcx_conjunction_pairs (D > 0: d = p_cat - p_sat;
 * D = 0: d = p_hi - p_lo); q_m = +inf ("absent") where either object has a NaN among the six values of either end.  Interval m
 * holds an EVENT iff
 *   q_m < +inf,  q_m < q_m-1 (strictly),  q_m <= q_m+1,
 * where a neighbour that is absent or does not exist (m = 0, m = M-2) counts as +inf.  A minimum exactly on a grid node is seen by
 * both adjoining intervals with the same bits; the strict / non-strict pair gives it to the earlier one, once.
 * The threshold is applied to the events, afterwards, with the screens' comparison: sqrt(q_m) <= threshold.  threshold <= 0 keeps
 * every event.
 * An event is an EDGE event when the distance is still falling where the pair's common span ends: interval m has no valid left
 * neighbour and t_m is the interval's first instant, or no valid right neighbour and t_m is its last instant (those times are
 * assigned, not computed: the comparison is exact).  Edge events are reported and flagged, not dropped -- the screens list such
 * minima too.
 * Two things follow.  The event of a pair with the smallest distance, the earliest of equal ones, taken at threshold <= 0, carries
 * bit for bit the distance and time mpcx_conjunction_pairs returns for the pair (both order by (q, interval), and the earliest of
 * the equal smallest is strictly below its left neighbour).  (i, j) and (j, i) give the same events.
 *
 * mpcx_conjunction_events: pairs, S, D, M, eph, cat, T0, T1 as mpcx_conjunction_pairs takes them; max_events = E >= 1 slots per pair.
 *   events [n][E][4]  rows (i, j, distance in m, time in s), i and j as given: the pair's events in ascending interval order, which
 *                     is ascending time -- the EARLIEST E of them when there are more
 *   info   [n][E][2]  int32 (grid interval, 1 for an edge event else 0)
 *   count  [n]        int32: the events found (at or below the threshold), which may exceed E: a list that was cut off shows
 *   status [n]        MPCX_ST_OK (a pair without a valid interval has count 0); MPCX_ST_BADK for an index that is not a whole number
 *                     inside its side, or i == j with D = 0: count 0, and the other rows are not affected
 * The slots from min(count, E) on are written too: (i, j, NaN, NaN) and (-1, 0), so every byte of the outputs is defined.
 * n = 0 is a successful call that does nothing.  n < 0, S < 1, D < 0, M < 2, T1 <= T0, max_events < 1, a NaN threshold, a missing
 * array, cat given with D = 0 or missing with D > 0: MPCX_E_BADARG, nothing enqueued.  The host variant takes host pointers; the
 * _dev variant device pointers throughout, no workspace, and enqueues one kernel on `stream`.
 *
 * mpcx_conjunction_events_traj: from trajectories, argument for argument as mpcx_conjunction_pairs_traj; eph_status, cat_status and
 * the _dev variant's workspace of mpcx_conjunction_events_workspace_bytes(S, D, M) bytes likewise.  Same bits as
 * mpcx_ephemeris_batch followed by mpcx_conjunction_events.
 */
size_t mpcx_conjunction_events_workspace_bytes(int S, int D, int M);
int mpcx_conjunction_events(mpcx_ctx *ctx, int n, const double *pairs, int S, int D, int M, const double *eph, const double *cat,
                            double T0, double T1, double threshold, int max_events, double *events, int32_t *info, int32_t *count,
                            int32_t *status);
int mpcx_conjunction_events_dev(mpcx_ctx *ctx, int n, const double *pairs, int S, int D, int M, const double *eph, const double *cat,
                                double T0, double T1, double threshold, int max_events, double *events, int32_t *info,
                                int32_t *count, int32_t *status, void *stream);
int mpcx_conjunction_events_traj(mpcx_ctx *ctx, int n, const double *pairs, int S, int nn, const int32_t *ns, const double *Y,
                                 const double *units, const double *span, int D, int cat_n, const int32_t *cat_ns,
                                 const double *cat_Y, const double *cat_units, const double *cat_span, int M, double T0, double T1,
                                 double threshold, int max_events, double *events, int32_t *info, int32_t *count, int32_t *status,
                                 int32_t *eph_status, int32_t *cat_status);
int mpcx_conjunction_events_traj_dev(mpcx_ctx *ctx, int n, const double *pairs, int S, int nn, const int32_t *ns, const double *Y,
                                     const double *units, const double *span, int D, int cat_n, const int32_t *cat_ns,
                                     const double *cat_Y, const double *cat_units, const double *cat_span, int M, double T0,
                                     double T1, double threshold, int max_events, double *events, int32_t *info, int32_t *count,
                                     int32_t *status, int32_t *eph_status, int32_t *cat_status, void *workspace, void *stream);

/*
 * The close approach of a listed row NEAREST THE ROW'S OWN TIME: an encounter followed through re-screens.  mpcx_conjunction_pairs
 * returns a pair's global minimum, so after a manoeuvre every row of a pair that mpcx_conjunction_events listed several times reads
 * the same encounter; these calls return, for every row, the encounter the row was listed for.
 *
 * The definition.  Rows are (i, j, -, t_row) on the grid linspace(T0, T1, M); columns 0, 1 and 3 are read.  An event is exactly
 * mpcx_conjunction_events' event WITHOUT a threshold (the caller needs the distance of an encounter that a manoeuvre has opened
 * beyond any): interval m holds one iff q_m < +inf, q_m < q_m-1 and q_m <= q_m+1, an absent neighbour counting as +inf, with (q_m,
 * t_m) of interval m alone and the operands of mpcx_conjunction_pairs.  The row's answer is the event that minimises the key
 * (|t_m - t_row|, m) -- a total order: of two events equally far from t_row the one in the earlier interval.  max_shift (seconds)
 * > 0 admits only events with |t_m - t_row| <= max_shift; max_shift <= 0 is unlimited.
 *   out    [n][4]  (i, j, distance in m, time in s) in list order, i and j as given
 *   info   [n][2]  int32 (grid interval, 1 for an edge event else 0), mpcx_conjunction_events' edge rule; may be NULL
 *   status [n]     MPCX_ST_OK, or MPCX_ST_BADK
 * A row with no event, or none within max_shift: (i, j, +inf, NaN), info (-1, 0), MPCX_ST_OK -- mpcx_conjunction_pairs' row without
 * a valid interval.  An index that is not a whole number inside its side, i == j with D = 0, or a t_row that is NaN or infinite:
 * (i, j, NaN, NaN), info (-1, 0), MPCX_ST_BADK, and the other rows are not affected.  A finite t_row outside [T0, T1] is a time
 * like any other: it picks the first or the last event.  Every byte of the outputs is defined.
 * Two things follow.  A row of mpcx_conjunction_events' output, given back on the same inputs, returns its own distance, time,
 * interval and edge flag bit for bit (its |t_m - t_row| is 0, and two events never share a time); so does a row of
 * mpcx_conjunction_pairs' output.  (i, j) and (j, i) give the same bits.
 * n = 0 is a successful call that does nothing.  n < 0, S < 1, D < 0, M < 2, T1 <= T0, a NaN max_shift, a missing pairs, eph, out
 * or status, cat given with D = 0 or missing with D > 0: MPCX_E_BADARG with "conjunction_track" in the message, nothing enqueued.
 * The host variant takes host pointers; the _dev variant device pointers throughout, no workspace, and enqueues one kernel on
 * `stream`.
 *
 * mpcx_conjunction_track_traj: from trajectories, argument for argument as mpcx_conjunction_pairs_traj; eph_status, cat_status and
 * the _dev variant's workspace of mpcx_conjunction_track_workspace_bytes(S, D, M) bytes (= mpcx_conjunction_pairs_workspace_bytes)
 * likewise.  Same bits as mpcx_ephemeris_batch followed by mpcx_conjunction_track.
 */
size_t mpcx_conjunction_track_workspace_bytes(int S, int D, int M);
int mpcx_conjunction_track(mpcx_ctx *ctx, int n, const double *pairs, int S, int D, int M, const double *eph, const double *cat,
                           double T0, double T1, double max_shift, double *out, int32_t *info, int32_t *status);
int mpcx_conjunction_track_dev(mpcx_ctx *ctx, int n, const double *pairs, int S, int D, int M, const double *eph, const double *cat,
                               double T0, double T1, double max_shift, double *out, int32_t *info, int32_t *status, void *stream);
int mpcx_conjunction_track_traj(mpcx_ctx *ctx, int n, const double *pairs, int S, int nn, const int32_t *ns, const double *Y,
                                const double *units, const double *span, int D, int cat_n, const int32_t *cat_ns,
                                const double *cat_Y, const double *cat_units, const double *cat_span, int M, double T0, double T1,
                                double max_shift, double *out, int32_t *info, int32_t *status, int32_t *eph_status,
                                int32_t *cat_status);
int mpcx_conjunction_track_traj_dev(mpcx_ctx *ctx, int n, const double *pairs, int S, int nn, const int32_t *ns, const double *Y,
                                    const double *units, const double *span, int D, int cat_n, const int32_t *cat_ns,
                                    const double *cat_Y, const double *cat_units, const double *cat_span, int M, double T0,
                                    double T1, double max_shift, double *out, int32_t *info, int32_t *status, int32_t *eph_status,
                                    int32_t *cat_status, void *workspace, void *stream);

/*
 * Collision probability of screened pairs.  A miss distance alone says nothing: the two orbit uncertainties decide whether 200 m
 * is an emergency or noise.  Two steps, both on the device: a covariance propagated along every trajectory, and for every row
 * (i, j, distance, time) of a screen's pairs list the short-encounter collision probability in the encounter plane.  The reference
 * carries no covariance anywhere.
 *
 * mpcx_covariance_batch: the covariance of position (m) and velocity (m/s) at every node of S trajectories.
 *   X [S][7][K] normalised trajectories (rows of length K, Ks[s] nodes in use; Ks = NULL: all K; the ragged convention above),
 *   U [S][3][K] the thrust at the nodes (NULL: zero thrust), units [S][2], span [S][2] as mpcx_ephemeris_batch takes them,
 *   consts [S][MPCX_NCONST], flags = MPCX_FLAG_DRAG | MPCX_FLAG_J2 | MPCX_FLAG_ATMO with the meaning they have on the discretize
 *   entry points (any other bit: MPCX_E_BADARG), max_step the discretiser's,
 *   P0 [S][6][6] the covariance at the first node (only its upper triangle is read), q [S] white acceleration noise in m^2/s^3
 *   (NULL: 0)  ->  P [S][K][6][6], status [S].
 * Per satellite: tf = (span[1] - span[0]) / units[1]; the library linearises about (X, U, tf) with
 * mpcx_discretize_stages_ragged_dev (Ku = K, Kus = Ks); Phi_k is the upper-left 6 x 6 block of interval k's stage record A.  That
 * is exact, not an approximation: the mass row of A is zero in the position and velocity columns, and the mass variance is held
 * at zero, so the 7 x 7 chain restricted to position and velocity IS the 6 x 6 chain.  In physical units Phi~_k = D Phi_k D^-1,
 * D = diag(L, L, L, V, V, V), V = L / Tu;  P_0 = P0,  P_k+1 = Phi~_k P_k Phi~_k^T + q Q(h),
 * Q(h) = [[h^3/3 I, h^2/2 I], [h^2/2 I, h I]], h = (span[1] - span[0]) / (Ks[s] - 1) the node spacing in seconds.  The upper
 * triangle is computed and mirrored: P is symmetric to the bit.
 * status: Ks[s] outside 2..K, span[1] <= span[0], or a tf that is not positive and finite (a time unit that is zero, negative or not
 * finite): MPCX_ST_BADK; a discretiser status other than MPCX_ST_OK is passed on; a
 * non-finite P0: MPCX_ST_NUMERIC.  In all three cases that satellite's P is NaN in all K nodes and the other satellites are
 * untouched.  Otherwise the nodes past Ks[s] come back zero.  S < 1, K < 2, max_step <= 0, an unknown flag, MPCX_FLAG_ATMO
 * without drag or without an atmosphere on the context: MPCX_E_BADARG, nothing enqueued.
 * The _dev variant takes device pointers throughout and a workspace of mpcx_covariance_workspace_bytes(S, K) bytes (the stage
 * records, tf, the zero thrust table, the discretiser's status; 0 for S < 1 or K < 2; contents unspecified on entry and exit).
 */
size_t mpcx_covariance_workspace_bytes(int S, int K);
int mpcx_covariance_batch(mpcx_ctx *ctx, int S, int K, const int32_t *Ks, const double *X, const double *U, const double *units,
                          const double *span, const double *consts, int flags, double max_step, const double *P0, const double *q,
                          double *P, int32_t *status);
int mpcx_covariance_batch_dev(mpcx_ctx *ctx, int S, int K, const int32_t *Ks, const double *X, const double *U, const double *units,
                              const double *span, const double *consts, int flags, double max_step, const double *P0,
                              const double *q, double *P, int32_t *status, void *workspace, void *stream);

/*
 * mpcx_covariance_thrust_batch: mpcx_covariance_batch with a third source of uncertainty, the execution error of the thrust (the
 * Gates model: magnitude and pointing errors, each with a fixed and a proportional part).  mpcx_covariance_batch treats the thrust
 * table as known exactly; after a burn its execution error is the dominant new uncertainty, and a burn sized to "4 sigma" under a
 * perfect-execution covariance is not a 4-sigma burn.  Arguments as mpcx_covariance_batch, with U required, and
 *   exec [S][MPCX_NEXEC] = (s_fm, s_pm, s_fp, s_pp, u_off) per satellite, m_var0 [S] the mass variance at the first node in the
 *   satellite's own mass unit squared (NULL: 0)  ->  P [S][K][6][6], Pm [S][K][7] (optional, NULL: not returned), status [S].
 * Execution error at a node.  The executed thrust at node k is u_k + e_k; the e_k are independent between nodes, zero-mean and
 * Gaussian, and between nodes the error is interpolated by the same first-order hold as the plan -- the discretisation the stage
 * records already describe, x_k+1 = A_k x_k + B_kn[k] u_k + B_kp[k] u_k+1.  With u^ = u_k / |u_k|:
 *   Sigma_k = s_par^2 u^ u^T + s_perp^2 (I - u^ u^T),  s_par^2 = s_fm^2 + (s_pm |u_k|)^2,  s_perp^2 = s_fp^2 + (s_pp |u_k|)^2.
 * s_fm, s_fp and u_off are in the satellite's own normalised thrust unit, as U is; s_pm is a fraction; s_pp is in radians, per
 * transverse axis.  A node with |u_k| <= u_off (or a |u_k| that is not a number) has Sigma_k = 0: the engine is off there, so there
 * is no error and no direction is needed.  u_off >= 0 is required.
 * The chain runs over all seven states -- a thrust error changes the mass flow, and a mass error changes later accelerations through
 * A[3:6][6] -- in the units of mpcx_covariance_batch extended by the mass, which stays in the satellite's own mass unit:
 * D = diag(L, L, L, V, V, V, 1), V = L / Tu; Phi~_k = D A_k D^-1, Bn~ = D B_kn[k], Bp~ = D B_kp[k].  x_k is correlated with e_k,
 * because e_k entered the previous interval through B_kp, so the 7 x 3 cross-covariance C_k = Cov(x_k, e_k) is carried:
 *   P_0 = [[P0, 0], [0, m_var0]],  C_0 = 0,
 *   Y     = (Phi~_k C_k) Bn~^T,
 *   P_k+1 = ((((Phi~_k P_k) Phi~_k^T + (Y + Y^T)) + (Bn~ Sigma_k) Bn~^T) + (Bp~ Sigma_k+1) Bp~^T) + q Q(h),
 *   C_k+1 = Bp~ Sigma_k+1,
 * q Q(h) on the 6 x 6 block as in mpcx_covariance_batch.  Sums run their index in ascending order; entry (i, j) is computed as entry
 * (min, max) and mirrored, so P is symmetric to the bit.
 * P is the position / velocity block (m, m/s), which every consumer of mpcx_covariance_batch's P takes unchanged; Pm is row 6 of the
 * 7 x 7: the mass covariances with position and velocity, and the mass variance.
 * The zero case is mpcx_covariance_batch, to the bit: for a satellite whose exec row is all zero and whose m_var0 is 0, every added
 * term is an exact zero and the seventh term of each product is x * 0, and the 6-term prefix of each sum is written as
 * mpcx_covariance_batch's kernel writes it (a zero may differ in sign).  That holds per satellite inside a mixed batch; no
 * satellite is handed to the other kernel.
 * status: mpcx_covariance_batch's, in its order; then a negative or non-finite exec entry, or a negative or non-finite m_var0:
 * MPCX_ST_NUMERIC.  A failed satellite is NaN in P and Pm at all K nodes and the other satellites are untouched; otherwise the nodes
 * past Ks[s] come back zero.  S < 1, K < 2, max_step <= 0, an unknown flag, MPCX_FLAG_ATMO without drag or without an atmosphere on
 * the context, or a NULL X, U, units, span, consts, P0, exec, P or status: MPCX_E_BADARG with "covariance_thrust" in the message,
 * nothing enqueued.
 * The _dev variant takes device pointers throughout and a workspace of mpcx_covariance_thrust_workspace_bytes(S, K) bytes (the stage
 * records, tf, the discretiser's status; 0 for S < 1 or K < 2; contents unspecified on entry and exit).
 */
#define MPCX_NEXEC 5
size_t mpcx_covariance_thrust_workspace_bytes(int S, int K);
int mpcx_covariance_thrust_batch(mpcx_ctx *ctx, int S, int K, const int32_t *Ks, const double *X, const double *U, const double *units,
                                 const double *span, const double *consts, int flags, double max_step, const double *P0, const double *q,
                                 const double *exec, const double *m_var0, double *P, double *Pm, int32_t *status);
int mpcx_covariance_thrust_batch_dev(mpcx_ctx *ctx, int S, int K, const int32_t *Ks, const double *X, const double *U,
                                     const double *units, const double *span, const double *consts, int flags, double max_step,
                                     const double *P0, const double *q, const double *exec, const double *m_var0, double *P, double *Pm,
                                     int32_t *status, void *workspace, void *stream);

/*
 * mpcx_covariance_drag_batch: mpcx_covariance_thrust_batch with a fourth source of uncertainty, the drag.  The other chains treat
 * the drag as known exactly; over several revolutions the error of the atmospheric density together with the ballistic coefficient
 * (typically 10-30 %) is the largest uncertainty of a low orbit, it grows along-track roughly quadratically with time, and white
 * acceleration noise q cannot imitate it.  Arguments as mpcx_covariance_thrust_batch, with
 *   flags containing MPCX_FLAG_DRAG (the drag is always in the model), exec optional (NULL: all-zero rows, no execution error),
 *   dens [S][MPCX_NDENS] = (sigma_b, tau_b) per satellite  ->  P [S][K][6][6], Pm [S][K][7] (optional), Pb [S][K][8] (optional,
 *   NULL: not returned), status [S].
 * The model.  The drag acceleration of satellite s is (1 + beta) a_D; beta, the fractional error of rho C_D S / m, is a zero-mean
 * scalar, independent of the initial state, of the thrust errors and of q: a first-order Gauss-Markov process with stationary
 * variance sigma_b^2 and correlation time tau_b in seconds, held constant over each node interval:
 *   beta_k+1 = phi beta_k + w_k,  phi = exp(-h / tau_b),  Var w_k = (1 - phi^2) sigma_b^2,  h the node spacing in seconds.
 * tau_b = +inf is a constant bias (the classical consider parameter): phi = 1 exactly.
 * The chain runs over z = (position, velocity, mass, beta).  The library linearises once, with MPCX_FLAG_DRAG_COLUMN, so that every
 * record carries G_k = d x_k+1 / d beta; with D, Phi~, Bn~, Bp~, Sigma_k, C_k of mpcx_covariance_thrust_batch and G~ = D G_k:
 *   Phi8  = [[Phi~_k, G~], [0, phi]],   P8_0 = diag(P0, m_var0, sigma_b^2),
 *   P8_k+1 = (((((Phi8 P8_k) Phi8^T + (Y + Y^T)) + (Bn~ Sigma_k) Bn~^T) + (Bp~ Sigma_k+1) Bp~^T) + q Q(h)) + (1 - phi^2) sigma_b^2 e_7 e_7^T,
 * the thrust terms on the 7 x 7 block (the beta row of C_k is zero and is not carried), q Q(h) on the 6 x 6 block.  Sums run their
 * index in ascending order -- the seven terms of mpcx_covariance_thrust_batch's sums first, written as its kernel writes them, the
 * beta term last; entry (i, j) is computed as entry (min, max) and mirrored, so P is symmetric to the bit.
 * P is the position / velocity block (m, m/s), unchanged in meaning: every consumer takes it as is.  Pm is row 6 of the 8 x 8 (its
 * first 7 entries), as in mpcx_covariance_thrust_batch.  Pb is row 7: Cov(beta_k, position) in m, Cov(beta_k, velocity) in m/s,
 * Cov(beta_k, mass) and Var beta_k.
 * The zero case is mpcx_covariance_thrust_batch, to the bit: for a satellite with sigma_b = 0 row and column 7 of P8 stay exact
 * zeros, every beta term is x * 0, and P and Pm have that call's bits under the same flags (a zero may differ in sign), per
 * satellite inside a mixed batch; with an all-zero exec row and m_var0 = 0 as well they are mpcx_covariance_batch's.
 * Not modelled: a density error common to both objects of a pair.  Two satellites of one shell see nearly the same density error,
 * which largely cancels in their relative position; consumers that add P_i + P_j as independent overstate the relative covariance
 * of such a pair.  Pb is returned so that a caller can form the cross term.
 * status: mpcx_covariance_thrust_batch's, in its order; then a negative or non-finite sigma_b, or a tau_b that is <= 0 or NaN
 * (+inf is valid): MPCX_ST_NUMERIC.  A failed satellite is NaN in P, Pm and Pb at all K nodes and the other satellites are
 * untouched; otherwise the nodes past Ks[s] come back zero.  S < 1, K < 2, max_step <= 0, an unknown flag (MPCX_FLAG_DRAG_COLUMN is
 * one here), a missing MPCX_FLAG_DRAG, MPCX_FLAG_ATMO without an atmosphere on the context, or a NULL X, U, units, span, consts, P0,
 * dens, P or status: MPCX_E_BADARG with "covariance_drag" in the message, nothing enqueued.
 * The _dev variant takes device pointers throughout and a workspace of mpcx_covariance_drag_workspace_bytes(S, K) bytes (the stage
 * records, tf, the discretiser's status; 0 for S < 1 or K < 2; contents unspecified on entry and exit).
 */
#define MPCX_NDENS 2
size_t mpcx_covariance_drag_workspace_bytes(int S, int K);
int mpcx_covariance_drag_batch(mpcx_ctx *ctx, int S, int K, const int32_t *Ks, const double *X, const double *U, const double *units,
                               const double *span, const double *consts, int flags, double max_step, const double *P0, const double *q,
                               const double *exec, const double *m_var0, const double *dens, double *P, double *Pm, double *Pb,
                               int32_t *status);
int mpcx_covariance_drag_batch_dev(mpcx_ctx *ctx, int S, int K, const int32_t *Ks, const double *X, const double *U,
                                   const double *units, const double *span, const double *consts, int flags, double max_step,
                                   const double *P0, const double *q, const double *exec, const double *m_var0, const double *dens,
                                   double *P, double *Pm, double *Pb, int32_t *status, void *workspace, void *stream);

/*
 * mpcx_collision_probability: pairs [n][4] rows exactly as the screens write them, (i, j, distance, time in s); the distance is
 * not read.  The row side: S, K, Ks, Y [S][7][K], units, span (as mpcx_ephemeris_batch takes them), P [S][K][6][6] (m, m/s:
 * mpcx_covariance_batch's), radius [S] the hard-body radius in m.  The column side: the same eight arguments with D.  cat_Y = NULL:
 * the columns are the rows (the all-pairs screen: j indexes the constellation; the other cat_ arguments are ignored); otherwise j
 * indexes the catalogue, as in mpcx_conjunction_cross_screen.  mu in m^3/s^2.
 * Each object of a pair at the pair's time t: position and velocity from the cubic Hermite on its own nodes, exactly
 * mpcx_ephemeris_batch's formulas (u = (t - t_a) / h_n, k = clamp(floor u, 0, ns - 2), s = u - k).  The nearest node is
 * kc = k + (s >= 0.5), dt = t - (t_a + kc h_n); with r the position at node kc in metres, G = mu (3 r r^T - |r|^2 I) / |r|^5, the
 * position rows of the short-arc transition are Phi_r = [ I + G dt^2/2 | dt I + G dt^3/6 ] and the position covariance at t is
 * C = Phi_r P_kc Phi_r^T (first neglected term: order (n dt)^3, n the mean motion).  An index outside its side, a node count
 * outside 2..K, an empty span or t outside the span: MPCX_ST_BADK.
 * The pair: d = p_b - p_a, w = v_b - v_a; |w| zero or not finite, or R = radius_a + radius_b not finite: MPCX_ST_NUMERIC.  e_w = w / |w|, m = d - (d . e_w) e_w,
 * e_1 = m / |m| (|m| = 0: the coordinate axis on which |e_w| is smallest, made orthogonal to e_w and normalised), e_2 = e_w x e_1,
 * C_2 = E^T (C_a + C_b) E with E = [e_1 e_2]; eigenvalues l_1 >= l_2 of C_2 and phi = 1/2 atan2(2 c_12, c_11 - c_22) in closed
 * form; l_2 <= 0 or not finite: MPCX_ST_NUMERIC.  In the principal frame the miss is (x_m, y_m) = (|m| cos phi, -|m| sin phi),
 * sigma_i = sqrt(l_i), R = radius_a + radius_b (R <= 0: probability 0), and
 *   Pc = int_-R^R 1/2 [erf((y_m + c(x)) / (sqrt 2 sigma_2)) - erf((y_m - c(x)) / (sqrt 2 sigma_2))]
 *                 exp(-1/2 ((x - x_m) / sigma_1)^2) / (sqrt(2 pi) sigma_1) dx,   c(x) = sqrt(R^2 - x^2),
 * the Gaussian's integral over the disc of radius R, by x = R sin theta and the 64-point Gauss-Legendre rule on [-pi/2, pi/2]
 * (the substitution's factor R cos theta removes the end-point singularity), clamped to [0, 1].
 * Accuracy domain of the fixed rule (against an adaptive double integral, misses up to 3 sigma, axis ratios up to 10): relative
 * error 1e-13 or better for R / sigma_2 <= 2, 3e-9 at 4, 2e-6 at 8, 6e-3 at 20.  Operational encounters have sigma of tens of
 * metres to kilometres and R of metres; there is no adaptive rule.
 * out [n][MPCX_NPC] (MPCX_PC_*), status [n]; a pair whose status is not MPCX_ST_OK has NaN in all six columns; the other pairs are
 * untouched by it.  n < 1, S < 1, K < 2, mu <= 0, a catalogue with D < 1 or cat_K < 2: MPCX_E_BADARG, nothing enqueued.
 * The _dev variant takes device pointers throughout and needs no workspace.
 */
enum { MPCX_PC_P = 0,       /* collision probability */
       MPCX_PC_MISS,        /* |m|: the miss distance in the encounter plane, m */
       MPCX_PC_SPEED,       /* |w|: the relative speed, m/s */
       MPCX_PC_SIGMA1,      /* sqrt(l_1), m */
       MPCX_PC_SIGMA2,      /* sqrt(l_2), m */
       MPCX_PC_MAHAL,       /* sqrt(x_m^2 / l_1 + y_m^2 / l_2) */
       MPCX_NPC };
int mpcx_collision_probability(mpcx_ctx *ctx, int n, const double *pairs, int S, int K, const int32_t *Ks, const double *Y,
                               const double *units, const double *span, const double *P, const double *radius, int D, int cat_K,
                               const int32_t *cat_Ks, const double *cat_Y, const double *cat_units, const double *cat_span,
                               const double *cat_P, const double *cat_radius, double mu, double *out, int32_t *status);
int mpcx_collision_probability_dev(mpcx_ctx *ctx, int n, const double *pairs, int S, int K, const int32_t *Ks, const double *Y,
                                   const double *units, const double *span, const double *P, const double *radius, int D,
                                   int cat_K, const int32_t *cat_Ks, const double *cat_Y, const double *cat_units,
                                   const double *cat_span, const double *cat_P, const double *cat_radius, double mu, double *out,
                                   int32_t *status, void *stream);

/*
 * mpcx_collision_probability_window: the collision probability of listed rows over a time window, for encounters the
 * short-encounter model above does not cover.  That model takes the relative motion as a straight line, freezes both position
 * covariances at the pair's time, ignores velocity uncertainty and integrates in the plane across the relative velocity: right for
 * crossing orbits at km/s, wrong for neighbours in one shell or satellites deployed together, which pass at cm/s to m/s over minutes
 * to a revolution (at zero relative speed it has no plane at all: MPCX_ST_NUMERIC).  This call has no encounter plane.
 * Arguments: those of mpcx_collision_probability, then half_window [n] in seconds and panels (1 .. MPCX_PW_MAX_PANELS).
 * Per row (i, j, ., t) the window is [t_a, t_b] = [t - h, t + h] cut to both objects' spans.  Index, node count, span and t are tested
 * as above, on both objects at t (MPCX_ST_BADK); h not positive and finite, or t_b <= t_a: MPCX_ST_BADK; R = radius_i + radius_j not
 * finite: MPCX_ST_NUMERIC; R <= 0: P, START, ENTRIES and RATE_MAX are 0, T_RATE_MAX = t_a, status MPCX_ST_OK, no covariance is read.
 * The model.  At a time tau the relative state (rho, nu) is Gaussian with mean (d, w) = (p_b - p_a, v_b - v_a) -- the cubic Hermite
 * on each object's own nodes and its derivative, as above -- and covariance [[A, B^T], [B, D]] = the sum of the two objects' 6 x 6
 * covariances, each carried from its nearest node over dt by the short-arc transition with its velocity rows, Sigma = Phi P_kc Phi^T,
 *   Phi = [[I + G0 dt^2/2, dt I + G0 dt^3/6], [(G0 + 4 Gm + Ge) dt/6 + G0^2 dt^3/6, I + (2 Gm + Ge) dt^2/6]].
 * The position rows, and with them A, are mpcx_collision_probability's C to the letter: G0 is the gradient at the node, the first
 * neglected term G' dt^3/6, order (n dt)^3 in units of the mean motion n.  The velocity rows are their derivative, int_0^dt G(s)
 * Phi_r(s) ds, by Simpson's rule on the gradient at the node, at the middle (Gm) and at the end (Ge) of the arc, the positions there
 * r + v s + a s^2/2 from the node's own velocity v and two-body acceleration a = -mu r / |r|^3; they neglect order (n dt)^4.  (With
 * the node's gradient alone, [G0 dt, I + G0 dt^2/2], the velocity-position block neglects G' dt^2/2, order (n dt)^2.)  Measured
 * against a finite-difference transition at half a node interval, eccentricity 0.15: the whole matrix is off by 7.3e-4 relative at
 * 31 nodes per revolution ((n dt)^3 = 1.15e-3) and 2.0e-5 at 101 (3.1e-5); the velocity rows alone by 1.4e-4 and 1.2e-6.
 * The rate at which probability enters the sphere |rho| = R is (Rice; Coppola), with x = R n - d on the unit sphere,
 *   rate(tau) = R^2 oint N_3(R n; d, A) E[(-n . nu)^+ | rho = R n] dOmega,   E = s phi(v0 / s) - v0 Phi(-v0 / s),
 *   v0 = n . (w + B A^-1 x),   s^2 = n^T (D - B A^-1 B^T) n   (s^2 <= 0: E = max(-v0, 0)),
 * evaluated through A = L L^T (closed form; a pivot that is not positive and finite at any time node, or a relative speed or a
 * result that is not finite: MPCX_ST_NUMERIC): z = L^-1 x, N_3 = (2 pi)^-3/2 exp(-|z|^2 / 2) / det L, B A^-1 x = W z with W = B L^-T,
 * D - B A^-1 B^T = D - W W^T.  The result is
 *   START + ENTRIES,   START = P(|rho(t_a)| <= R) (a ball integral),   ENTRIES = int_t_a^t_b rate dtau,
 * the probability of being inside at t_a plus the expected number of entries.  That is the probability of a collision in the
 * window exactly when no sample path enters the sphere twice in it, and an UPPER BOUND otherwise; P = min(1, START + ENTRIES).
 * Intended use: one window per event of mpcx_conjunction_events, joined per pair as independent events.
 * Fixed rules, no adaptivity.  Time: `panels` equal panels of [t_a, t_b], the 64-point Gauss-Legendre rule on each.  Sphere: the
 * pole along w(tau) (|w| = 0: the x axis), e_1 from the coordinate axis on which the pole's component is smallest (the |m| = 0 rule
 * above), e_2 = pole x e_1; cos theta split at the equator -- without velocity uncertainty the integrand has a kink on n . w = 0 --
 * with 8 Gauss-Legendre nodes on [-1, 0] and 8 on [0, 1], times 32 azimuths (k + 1/2) 2 pi / 32: 512 points.  Ball: 8
 * Gauss-Legendre radii on [0, R] times the same sphere rule, at t_a.
 * Accuracy domain of the rules (tests/test_collision_window_host.py).  Against mpcx_collision_probability's integral in its own
 * domain (7 km/s, no velocity uncertainty, window +-(8 sigma_max + R) / |w|, misses up to 2 sigma, anisotropic): relative error
 * 1.3e-14 for R / sigma_min <= 2 and 8.8e-7 at 4 with 4 panels, 4.7e-7 for R / sigma_min <= 2 with 1 panel.  Ball term against the
 * non-central chi-square (misses up to 3 sigma): 1.2e-15 for R / sigma <= 1, 2.1e-11 at 2.  A slow encounter with velocity
 * uncertainty (0.25 m/s over 1200 s, R = 30 m, sigma 40 .. 120 m) against 400 000 sampled straight paths: 0.045460 at 1, 2 and 4
 * panels, inside the sampling error 3.3e-4.  The window must resolve the rate: in those cases a panel is 4 (8 sigma_max + R) / |w|
 * long at 1 panel and a quarter of that at 4.
 * out [n][MPCX_NPW] (MPCX_PW_*), status [n]; a row whose status is not MPCX_ST_OK is NaN in every column; the other rows are
 * untouched by it.  n < 1, S < 1, K < 2, mu <= 0, a catalogue with D < 1 or cat_K < 2, panels outside 1 .. MPCX_PW_MAX_PANELS, a
 * required array NULL: MPCX_E_BADARG, nothing enqueued.  The _dev variant takes device pointers throughout and needs no workspace.
 */
enum { MPCX_PW_P = 0,       /* min(1, START + ENTRIES) */
       MPCX_PW_START,       /* P(|rho(t_a)| <= R) */
       MPCX_PW_ENTRIES,     /* the expected number of entries into the sphere over [t_a, t_b] */
       MPCX_PW_RATE_MAX,    /* the largest rate at a time node, 1/s */
       MPCX_PW_T_RATE_MAX,  /* its time (the earliest of equal ones), s */
       MPCX_PW_TA,          /* the window used, s */
       MPCX_PW_TB,
       MPCX_NPW };
enum { MPCX_PW_MAX_PANELS = 64 };
int mpcx_collision_probability_window(mpcx_ctx *ctx, int n, const double *pairs, int S, int K, const int32_t *Ks, const double *Y,
                                      const double *units, const double *span, const double *P, const double *radius, int D,
                                      int cat_K, const int32_t *cat_Ks, const double *cat_Y, const double *cat_units,
                                      const double *cat_span, const double *cat_P, const double *cat_radius, double mu,
                                      const double *half_window, int panels, double *out, int32_t *status);
int mpcx_collision_probability_window_dev(mpcx_ctx *ctx, int n, const double *pairs, int S, int K, const int32_t *Ks, const double *Y,
                                          const double *units, const double *span, const double *P, const double *radius, int D,
                                          int cat_K, const int32_t *cat_Ks, const double *cat_Y, const double *cat_units,
                                          const double *cat_span, const double *cat_P, const double *cat_radius, double mu,
                                          const double *half_window, int panels, double *out, int32_t *status, void *stream);

/*
 * mpcx_encounter_window: the time window of every listed row, chosen on the device -- the half_window that
 * mpcx_collision_probability_window, mpcx_collision_window_sensitivity, mpcx_avoidance_window, mpcx_avoidance_window_refine and
 * mpcx_collision_probability_mc take per row.  One rule whether the pair closes at km/s (a fraction of a second) or does not move at
 * all (minutes, or the whole span): outside the window the pair's MEAN separation is more than nsigma combined sigmas, plus the summed
 * radii, away from a collision.
 * Arguments: those of mpcx_collision_probability_window up to mu, then max_half [n] in seconds (how far from t the search may go, per
 * row), nsigma (positive and finite) and levels (1 .. MPCX_EW_MAX_LEVELS).
 * The rule.  At a time tau the node of mpcx_collision_probability_window (the same device function) gives the mean relative position d
 * and L^-1 of A = L L^T, the position block of the summed, carried 6 x 6 covariances.  With R = radius_i + radius_j,
 *   g(tau) = |L^-1 d| - max(R, 0) |L^-1|_F - nsigma,
 * |.|_F the Frobenius norm of the six stored entries of L^-1 summed row by row.  Since |L^-1|_F >= |L^-1|_2, g > 0 means that every
 * point of the sphere |rho| <= R -- every relative position that is a collision -- lies more than nsigma whitened units from the
 * mean d: |L^-1 (x - d)| >= |L^-1 d| - |L^-1|_2 |x|.  The rule is CONSERVATIVE on purpose: the Frobenius norm overstates the sphere by up to sqrt(3), so the window errs wide.
 * tau is LIVE when g(tau) <= 0.  A scan time outside either object's span is not live.  A scan time at which the node fails
 * numerically (a pivot of A not positive and finite, a relative speed that is not finite) cannot be ruled out: it counts as live and
 * sets MPCX_EW_BAD_SCAN in the row's flags, whether or not it ends up inside the window.
 * The search, for the side before t (sign -1), then for the side after it (sign +1), with H = max_half of the row: the bracket
 * [a, b] = [0, H] of offsets from t; `levels` times: wd = (b - a) / 64, cell end l = 0 .. 63 at the offset a + (l + 1) wd (one fused
 * multiply-add) is tested at t + sign offset, l* is the first that is not live, and [a, b] <- [a + l* wd, a + (l* + 1) wd].  No such
 * end at the first level: the side is OPEN, its reach is H and its search stops (MPCX_EW_OPEN_BEFORE / MPCX_EW_OPEN_AFTER: the live
 * stretch runs past max_half).  No such end at a later level: b stays and the search stops.  The side's reach is the final b, the
 * first offset known not to be live: the window errs wide by at most one final cell, H / 64^levels.  Only the connected live stretch
 * about t counts; a second approach of the same pair inside H is another row's (mpcx_conjunction_events lists it, and the caller
 * bounds max_half by the spacing to the neighbouring event).  g(t) > 0 -- t itself is not live --: the row is CLEAR
 * (MPCX_EW_CLEAR), nothing is searched and both reaches are H / 64^levels, so that every consumer still receives a positive window.
 * out [n][MPCX_NEW] (MPCX_EW_*), flags [n] (MPCX_EW_CLEAR | MPCX_EW_OPEN_BEFORE | MPCX_EW_OPEN_AFTER | MPCX_EW_BAD_SCAN), status [n]:
 * index, node count, span and t are tested on both objects at t as in mpcx_collision_probability_window (MPCX_ST_BADK); max_half not
 * positive and finite: MPCX_ST_BADK; R not finite, the node failing numerically at t itself, or a g(t) that is not finite:
 * MPCX_ST_NUMERIC.  A row whose status is not MPCX_ST_OK is NaN in every column with flags 0; the other rows are untouched by it.
 * One wave per row, 1 + 2 levels node evaluations per lane, no atomics: a row's result depends on its own arguments alone -- not on
 * the list's order or length, the launch or the device count.  n < 1, S < 1, K < 2, mu <= 0, a catalogue with D < 1 or cat_K < 2,
 * nsigma not positive and finite, levels outside 1 .. MPCX_EW_MAX_LEVELS, a required array NULL: MPCX_E_BADARG, nothing enqueued.
 * The _dev variant takes device pointers throughout and needs no workspace.
 */
enum { MPCX_EW_HALF = 0,        /* max(REACH_BEFORE, REACH_AFTER): what every half_window argument takes, s */
       MPCX_EW_TA,              /* t - REACH_BEFORE and t + REACH_AFTER, cut to both objects' spans, s */
       MPCX_EW_TB,
       MPCX_EW_REACH_BEFORE,    /* the first offset before t known not to be live (max_half: open), s */
       MPCX_EW_REACH_AFTER,     /* the same after t */
       MPCX_EW_G0,              /* g(t) */
       MPCX_NEW };
enum { MPCX_EW_CLEAR = 1,       /* flags: g(t) > 0, nothing searched */
       MPCX_EW_OPEN_BEFORE = 2, /* live all the way to t - max_half */
       MPCX_EW_OPEN_AFTER = 4,  /* live all the way to t + max_half */
       MPCX_EW_BAD_SCAN = 8 };  /* a scan time was numerically bad and counted as live */
enum { MPCX_EW_MAX_LEVELS = 4 };
int mpcx_encounter_window(mpcx_ctx *ctx, int n, const double *pairs, int S, int K, const int32_t *Ks, const double *Y,
                          const double *units, const double *span, const double *P, const double *radius, int D, int cat_K,
                          const int32_t *cat_Ks, const double *cat_Y, const double *cat_units, const double *cat_span,
                          const double *cat_P, const double *cat_radius, double mu, const double *max_half, double nsigma, int levels,
                          double *out, int32_t *flags, int32_t *status);
int mpcx_encounter_window_dev(mpcx_ctx *ctx, int n, const double *pairs, int S, int K, const int32_t *Ks, const double *Y,
                              const double *units, const double *span, const double *P, const double *radius, int D, int cat_K,
                              const int32_t *cat_Ks, const double *cat_Y, const double *cat_units, const double *cat_span,
                              const double *cat_P, const double *cat_radius, double mu, const double *max_half, double nsigma,
                              int levels, double *out, int32_t *flags, int32_t *status, void *stream);

/*
 * Avoidance manoeuvres for screened pairs from thrust sensitivities.  The screens say who comes close and when, the probability how
 * much that matters; this says what to change in the plan.  For every row (i, j, distance, time t in s) of a pairs list: the
 * derivative of the encounter-plane miss with respect to every thrust node of the plan (the B-plane sensitivity), by a backward
 * (adjoint) sweep over the stage records the discretiser integrates anyway, and from it the least-effort thrust change that opens
 * the miss to `target`.  Nothing in the reference does this.
 *
 * Inputs.  pairs [n][4] exactly as the screens write them (the distance is not read).  The row side is the constellation's plan,
 * as mpcx_covariance_batch takes it: S, K, Ks, Y [S][7][K], U [S][3][K] (required), units, span, consts, flags, max_step; P
 * [S][K][6][6] optional.  The column side D, cat_K, cat_Ks, cat_Y, cat_units, cat_span, cat_P: cat_Y = NULL means j indexes the
 * constellation (the all-pairs screen; the other cat_ arguments are ignored), otherwise the catalogue, as in
 * mpcx_collision_probability.  mu in m^3/s^2.  target > 0.  who: 0 the row object i manoeuvres, 1 object j, 2 both; 1 and 2 only
 * in the all-pairs form (a catalogue object is not ours to move).
 *
 * Linearisation: exactly mpcx_covariance_batch's -- tf = (span[1] - span[0]) / units[1], mpcx_discretize_stages_ragged_dev with
 * Ku = K, Kus = Ks, once per call for all S satellites, into the call's workspace.  The input convention is the reference's
 * (optimizer.py:334-335): x_k+1 = A_k x_k + B_kn[k] u_k + B_kp[k] u_k+1 + ..., B_kn multiplies the CURRENT node's thrust and B_kp
 * the NEXT node's (with the two swapped the sensitivities of a thrusting LEO arc miss central differences of the nonlinear flow by
 * 3.5 to 4.7 % of the largest entry instead of 0.24 to 0.35 %: tests/test_avoidance_host.py).  tf is held fixed: a thrust change
 * does not move the nodes' times.
 *
 * Encounter frame.  Both objects' position and velocity at t by the cubic Hermite on their own nodes (mpcx_ephemeris_batch's
 * formulas: u = (t - t_a) / h_n, k = clamp(floor u, 0, ns - 2), s = u - k), d = p_b - p_a, w = v_b - v_a, and e_w, e_1, e_2 exactly
 * as mpcx_collision_probability defines them, its |m| = 0 rule included.  In this frame the miss is (|m|, 0).
 *
 * Sensitivities of a manoeuvring object (7-state adjoint, normalised units).  L, Tu its units, h_tau = tf / (ns - 1), h00, h10,
 * h01, h11 the Hermite basis at s.  The library's own p(t) is linear in the two bracketing node states:
 *   Lam_k+1 = L [h01 I | h_tau h11 I | 0],  Lam_k = L [h00 I | h_tau h10 I | 0]   (3 x 7, metres),
 *   R = sgn [e_1 e_2 e_w]^T (3 x 3), sgn = -1 for object i (d = p_b - p_a), +1 for object j,
 *   lam_k+1 = R Lam_k+1,  lam_k = lam_k+1 A_k + R Lam_k,  lam_m = lam_m+1 A_m for m = k-1 .. 0,
 *   g_m = lam_m+1 B_kn[m] (m <= k) + lam_m B_kp[m-1] (1 <= m <= k+1):  3 x 3, metres per unit of normalised thrust at node m;
 * g_k+1 = lam_k+1 B_kp[k], g_0 = lam_1 B_kn[0], g_m = 0 for m > k + 1.  Every sum runs its index in ascending order.
 *
 * Effort metric (physical, so that satellites in different units can share one manoeuvre).  c_m = (L / Tu^2) / Y[6][m]: m/s^2
 * per unit of normalised thrust at node m; ghat_m = g_m / c_m; w_m = h_n seconds, halved at m = 0 and m = ns - 1 (the trapezoid
 * rule).  The authority matrix of the encounter-plane rows is M = sum_m ghat_m[0:2] ghat_m[0:2]^T / w_m (2 x 2, symmetric); with
 * who = 2, M = M_i + M_j.  det M <= 0 or a non-finite M: MPCX_ST_SINGULAR (no authority: t at the first node, say).
 *
 * Target metric.  With covariances W = C_2^-1, C_2 the combined 2 x 2 encounter-plane covariance exactly as
 * mpcx_collision_probability forms it (nearest node, short-arc rows): target is a Mahalanobis distance.  P = NULL (and cat_P = NULL
 * with a catalogue): W = I, target is a miss distance in metres.  One of P, cat_P without the other with a catalogue:
 * MPCX_E_BADARG.  d0 = sqrt(m^T W m).
 *
 * Manoeuvre.  d0 >= target: no change -- du, DM1, DM2, DT, DV_*, UMAX_* are 0, D1 = D0, MISS1 = |m|, status OK.  Otherwise the
 * encounter-plane displacement is dm = alpha p, p = M W (1, 0)^T: the direction in which m^T W m grows fastest per unit of effort;
 * alpha >= 0 the root of (m + alpha p)^T W (m + alpha p) = target^2 in the cancellation-free form alpha = -c / (b + sqrt(b^2 - a c))
 * (a = p^T W p, b = m^T W p, c = m^T W m - target^2).  With lambda = M^-1 dm every manoeuvring object gets
 * da_m = ghat_m[0:2]^T lambda / w_m (m/s^2) and du_m = da_m / c_m (normalised thrust, the plan's own units).  This du is the exact
 * least-effort (integral of |da|^2 dt, trapezoid rule) thrust change for that dm.  The DIRECTION is the first-order optimum, not
 * the optimum over the whole target ellipse: with W = I or M W a multiple of the identity the two coincide; with an anisotropic W
 * (axis ratio 10, the miss at 45 degrees to the axes) a scan over the ellipse finds a point that costs less -- by 5.4e-6 of the
 * effort on the test scene (tests/test_avoidance_host.py, profiles/avoidance.txt): there is a gap, and there it is small.
 *
 * Outputs.  out [n][MPCX_NAV] (MPCX_AV_*); du [n][NS][3][K], NS = 2 in the all-pairs form (slot 0 = i, 1 = j) and 1 with a
 * catalogue: nodes past k + 1 and the slot of an object that does not move are 0; sens [n][NS][3][3][K] (may be NULL: not written),
 * the g_m ordered row, thrust component, node.  du and out have the same bits with and without sens.  status [n]: MPCX_ST_BADK an
 * index outside its side, a node count outside 2..K, an empty span, t outside a span, a manoeuvring satellite without a positive
 * finite tf; MPCX_ST_NUMERIC whatever has that status in mpcx_collision_probability (|w| zero or not finite, l_2 <= 0 or not
 * finite); the discretiser's status of a manoeuvring satellite, passed on; MPCX_ST_SINGULAR as above.  A failed row is NaN in
 * out, du and sens; its neighbours are untouched.  n < 1, S < 1, K < 2, mu <= 0, target not a positive finite number, who outside
 * 0..2 or not 0 with a catalogue, max_step <= 0, an unknown flag or MPCX_FLAG_ATMO without drag or an atmosphere (as on
 * mpcx_covariance_batch): MPCX_E_BADARG, nothing enqueued.
 * The _dev variant takes device pointers throughout and a workspace of mpcx_avoidance_workspace_bytes(n, S, K) bytes (the stage
 * records, tf, the discretiser's status, the g_m when sens is NULL; 0 for n < 1, S < 1 or K < 2; contents unspecified on entry
 * and exit).  Results do not depend on the launch shape, on the block of rows a row is computed in, or on the device count.
 */
enum { MPCX_AV_D0 = 0,      /* d0: the distance now, in the target's metric */
       MPCX_AV_D1,          /* the predicted distance after the manoeuvre, in the target's metric */
       MPCX_AV_DM1,         /* dm in the (e_1, e_2) frame, m */
       MPCX_AV_DM2,
       MPCX_AV_MISS1,       /* |m + dm|, m */
       MPCX_AV_DT,          /* shift of the time of closest approach, -(e_w row of sum_m g_m du_m) / |w|, s */
       MPCX_AV_DV_I,        /* sum_m w_m |da_m| per object, m/s (0 for one that does not move) */
       MPCX_AV_DV_J,
       MPCX_AV_UMAX_I,      /* max_m |du_m| per object, to compare with u_max */
       MPCX_AV_UMAX_J,
       MPCX_NAV };
size_t mpcx_avoidance_workspace_bytes(int n, int S, int K);
int mpcx_avoidance(mpcx_ctx *ctx, int n, const double *pairs, int S, int K, const int32_t *Ks, const double *Y, const double *U,
                   const double *units, const double *span, const double *consts, int flags, double max_step, const double *P,
                   int D, int cat_K, const int32_t *cat_Ks, const double *cat_Y, const double *cat_units, const double *cat_span,
                   const double *cat_P, double mu, double target, int who, double *out, double *du, double *sens, int32_t *status);
int mpcx_avoidance_dev(mpcx_ctx *ctx, int n, const double *pairs, int S, int K, const int32_t *Ks, const double *Y, const double *U,
                       const double *units, const double *span, const double *consts, int flags, double max_step, const double *P,
                       int D, int cat_K, const int32_t *cat_Ks, const double *cat_Y, const double *cat_units, const double *cat_span,
                       const double *cat_P, double mu, double target, int who, double *out, double *du, double *sens,
                       int32_t *status, void *workspace, void *stream);

/*
 * mpcx_collision_window_sensitivity: mpcx_collision_probability_window together with its derivative with respect to every thrust
 * node of the object or objects that move.  mpcx_avoidance aims at a distance in the encounter plane; a slow pair has no such plane
 * (|w| = 0: MPCX_ST_NUMERIC there), and well before that the plane covariance has dropped what the window model carries.  This is
 * the derivative a target on the window probability needs.
 * Arguments: those of mpcx_collision_probability_window (P, radius and, with a catalogue, cat_P, cat_radius required) with the plan
 * side of mpcx_avoidance -- U, consts, flags, max_step -- and who (0 / 1 / 2: object i, object j, both; 1 and 2 only in the all-pairs
 * form).  Linearisation: mpcx_avoidance's, word for word -- one mpcx_discretize_stages_ragged_dev per call into the workspace, tf
 * fixed, x_k+1 = A_k x_k + B_kn[k] u_k + B_kp[k] u_k+1.
 * What is differentiated.  Q = START + ENTRIES, the unclamped sum (P = min(1, Q) is not).  The thrust moves only the MEAN relative
 * state (d(tau), w(tau)).  Held fixed: the node covariances and their short-arc carry, the window [t_a, t_b], the row's time, and the
 * sphere rule's pole (in the continuum the integral does not depend on it).  Neglected with that: the change of the carried
 * covariance with the moved node states, relative order (n dt)^2 |dr| / |r| through the gravity gradient of the short arc -- for a
 * manoeuvre of metres on an orbit of 7e6 m below 1e-6 of the covariance --, and the change the manoeuvre makes to the covariance's
 * own propagation (mpcx_covariance_batch is not run again: P is the caller's).
 * The state gradient.  With the notation above (x = R n - d, z = L^-1 x, W = B L^-T) and Phi = Phi(-v0 / s):
 *   dN_3/dd = N_3 L^-T z,   dE/dv0 = -Phi (s^2 <= 0: -1 where v0 < 0, else 0),   dv0/dw = n,   dv0/dd = -L^-T W^T n,
 * so that per point d(N_3 E)/dd = N_3 L^-T (E z + Phi W^T n) and d(N_3 E)/dw = -N_3 Phi n.  Per time node q, omega_q its weight
 * (half a panel's length times the Gauss-Legendre weight), with the sphere rule, radii and panels of the window call:
 *   c_q = omega_q R^2 cden [ L^-T sum wq dens (E z + Phi W^T n)  |  -sum wq dens Phi n ]     (1 x 6: d, then w),
 * the two sums run with the rate's, point by point in its order, and L^-T is applied once.  The ball term at t_a gives
 * dSTART/dd = cden L^-T (sum over the ball of N_3's weights times z), lanes and butterfly as for START, and nothing for w.
 * The adjoint sweep.  An object's position and velocity at tau are linear in its two bracketing node states (cp_state's Hermite;
 * h.., g.. the position's and the velocity's basis at s, h_n the node spacing in s, h_tau in the object's time unit, V = L / Tu):
 *   dp/dy_k = L [h00 I | h_tau h10 I | 0],  dv/dy_k = [(L g00 / h_n) I | V g10 I | 0],  node k+1 with h01, h11, g01, g11.
 * c_q puts sgn (c_q,d dp/dy + c_q,w dv/dy) on each of the two (sgn = -1 for object i, +1 for object j, as in mpcx_avoidance).  The
 * per-node sources sigma_m (1 x 7, the mass entry 0) are these shares summed over q in ascending order of q, the ball term last.  Then
 *   lam_ke+1 = sigma_ke+1 (ke the interval of the last time node),  lam_m = lam_m+1 A_m + sigma_m,
 *   g_m = lam_m+1 B_kn[m] (m <= ke) + lam_m B_kp[m-1] (1 <= m <= ke + 1),   g_m = 0 for m > ke + 1.
 * Outputs.  out [n][MPCX_NPW]: the bytes mpcx_collision_probability_window returns for the row.  sens [n][NS][3][K]: dQ/du_m per
 * unit of normalised thrust, NS = 2 in the all-pairs form (slot 0 = i, 1 = j) and 1 with a catalogue; 0 for an object that does not
 * move.  state_grad [n][64 panels + 1][6] (may be NULL; the other results have the same bits with and without it): the c_q, the ball
 * term last.  status [n]: the window call's statuses; then, for a row with a sphere, MPCX_ST_BADK for a manoeuvring satellite without
 * a positive finite tf and the discretiser's status of one, passed on.  A failed row is NaN in out, sens and state_grad; its
 * neighbours are untouched.  R <= 0: out as the window call gives it, sens = 0, state_grad = 0, MPCX_ST_OK, no mover is looked at.
 * Argument errors: the window call's and mpcx_avoidance's (who, max_step, flags), MPCX_E_BADARG, nothing enqueued.
 * The _dev variant takes device pointers throughout and a workspace of mpcx_collision_window_sensitivity_workspace_bytes(n, S, K,
 * panels) bytes (the stage records, tf, the discretiser's status, the node sources; 0 for n < 1, S < 1, K < 2 or panels outside
 * 1 .. MPCX_PW_MAX_PANELS; contents unspecified on entry and exit).  One wave per row, no atomics; results do not depend on the
 * launch shape, on the block of rows a row is computed in, or on the device count.
 */
size_t mpcx_collision_window_sensitivity_workspace_bytes(int n, int S, int K, int panels);
int mpcx_collision_window_sensitivity(mpcx_ctx *ctx, int n, const double *pairs, int S, int K, const int32_t *Ks, const double *Y,
                                      const double *U, const double *units, const double *span, const double *consts, int flags,
                                      double max_step, const double *P, const double *radius, int D, int cat_K, const int32_t *cat_Ks,
                                      const double *cat_Y, const double *cat_units, const double *cat_span, const double *cat_P,
                                      const double *cat_radius, double mu, const double *half_window, int panels, int who, double *out,
                                      double *sens, double *state_grad, int32_t *status);
int mpcx_collision_window_sensitivity_dev(mpcx_ctx *ctx, int n, const double *pairs, int S, int K, const int32_t *Ks, const double *Y,
                                          const double *U, const double *units, const double *span, const double *consts, int flags,
                                          double max_step, const double *P, const double *radius, int D, int cat_K,
                                          const int32_t *cat_Ks, const double *cat_Y, const double *cat_units, const double *cat_span,
                                          const double *cat_P, const double *cat_radius, double mu, const double *half_window, int panels,
                                          int who, double *out, double *sens, double *state_grad, int32_t *status, void *workspace,
                                          void *stream);

/*
 * mpcx_avoidance_window: for every listed row the thrust change of least effort, to first order, that brings the window
 * probability Q = START + ENTRIES down to target_p (strictly between 0 and 1).  Arguments: those of
 * mpcx_collision_window_sensitivity, then target_p, tol > 0 and max_eval >= 1.
 * Direction.  With mpcx_avoidance's effort metric (c_m, w_m, ghat_m = g_m / c_m, g_m the row's sens): steepest descent of Q per unit
 * of effort, da_m = -ghat_m / w_m and du_m(alpha) = alpha (da_m / c_m) for every object that moves.  Gamma = sum_m |ghat_m|^2 / w_m
 * (both movers with who = 2; per object lane-strided over the nodes, closed by the butterfly): to first order Q(alpha) = Q(0) -
 * alpha Gamma.  Gamma not positive and finite: MPCX_ST_SINGULAR -- a row whose two objects are one trajectory (d = 0: Q has a
 * stationary point there), a window that ends in the first node's reach of no thrust.
 * Only the dynamics are linearised, not the probability.  The response to du(1) is dx_0 = 0, dx_k+1 = A_k dx_k + B_kn[k] du_k +
 * B_kp[k] du_k+1, carried to every time node by the Hermite bases above with the sign sgn; Q(alpha) is the window rule -- all 64
 * panels x 512 points and the ball -- at the means (d + alpha dd, w + alpha dw) with the row's own covariances, frames (the pole of
 * the unmoved w) and rules.  Q(0) has mpcx_collision_probability_window's bits.
 * Step.  Q(0) <= target_p (tested first; a row without a sphere is there): du = 0, P1 = P0, everything else 0, MPCX_ST_OK.
 * Otherwise alpha_1 = Q(0) ln(Q(0) / target_p) / Gamma, the first-order step in ln Q; alpha is doubled until Q(alpha) <= target_p;
 * then the bracket [lo, hi] is closed on f = ln Q(alpha) - ln target_p by the Illinois rule: alpha = lo + (hi - lo) f_lo / (f_lo -
 * f_hi), replaced by the middle when it is not strictly inside the bracket; the end that is kept twice running has its f halved.
 * It stops at the first alpha with |f| <= tol, in either phase.  At most max_eval evaluations of Q(alpha), alpha > 0, are made:
 * without one left while doubling MPCX_ST_INFEASIBLE, while closing MPCX_ST_MAXITER.  An evaluation that is not finite:
 * MPCX_ST_NUMERIC.
 * Outputs.  out [n][MPCX_NAW] (MPCX_AW_*); du [n][NS][3][K] laid out as mpcx_avoidance's; sens [n][NS][3][K] (may be NULL) with
 * mpcx_collision_window_sensitivity's bits, whatever the manoeuvre's status; status [n]: that call's statuses, then the ones above.
 * A failed row is NaN in out and du; its neighbours are untouched.  target_p outside (0, 1), tol not positive and finite, max_eval <
 * 1 and whatever mpcx_collision_window_sensitivity refuses: MPCX_E_BADARG, nothing enqueued.  The _dev variant takes device
 * pointers throughout and a workspace of mpcx_avoidance_window_workspace_bytes(n, S, K, panels) bytes.  One wave per row; results
 * do not depend on the launch shape, on the block of rows a row is computed in, or on the device count.
 * Not done here: the covariances are not propagated again under the manoeuvre and the manoeuvre is not flown and corrected
 * (mpcx_avoidance_window_refine below does both), and these rows do not enter mpcx_avoidance_joint or mpcx_avoidance_refine (sens
 * is what they would need).
 */
enum { MPCX_AW_P0 = 0,      /* Q(0) = START + ENTRIES now (unclamped) */
       MPCX_AW_P1,          /* Q(alpha), the window rule at the moved means */
       MPCX_AW_ALPHA,       /* the step along the direction */
       MPCX_AW_DQ_LINEAR,   /* -alpha Gamma: the first-order prediction, to compare with P1 - P0 */
       MPCX_AW_DV_I,        /* sum_m w_m |da_m| per object, m/s (0 for one that does not move) */
       MPCX_AW_DV_J,
       MPCX_AW_UMAX_I,      /* max_m |du_m| per object, to compare with u_max */
       MPCX_AW_UMAX_J,
       MPCX_AW_EVALS,       /* evaluations of Q(alpha) made */
       MPCX_NAW };
size_t mpcx_avoidance_window_workspace_bytes(int n, int S, int K, int panels);
int mpcx_avoidance_window(mpcx_ctx *ctx, int n, const double *pairs, int S, int K, const int32_t *Ks, const double *Y, const double *U,
                          const double *units, const double *span, const double *consts, int flags, double max_step, const double *P,
                          const double *radius, int D, int cat_K, const int32_t *cat_Ks, const double *cat_Y, const double *cat_units,
                          const double *cat_span, const double *cat_P, const double *cat_radius, double mu, const double *half_window,
                          int panels, int who, double target_p, double tol, int max_eval, double *out, double *du, double *sens,
                          int32_t *status);
int mpcx_avoidance_window_dev(mpcx_ctx *ctx, int n, const double *pairs, int S, int K, const int32_t *Ks, const double *Y,
                              const double *U, const double *units, const double *span, const double *consts, int flags,
                              double max_step, const double *P, const double *radius, int D, int cat_K, const int32_t *cat_Ks,
                              const double *cat_Y, const double *cat_units, const double *cat_span, const double *cat_P,
                              const double *cat_radius, double mu, const double *half_window, int panels, int who, double target_p,
                              double tol, int max_eval, double *out, double *du, double *sens, int32_t *status, void *workspace,
                              void *stream);

/*
 * mpcx_avoidance_window_refine: mpcx_avoidance_window, then `rounds` times on the device: fly the manoeuvre, look at the row again
 * on what was flown, linearise about it and correct; then fly and look once more -- the answer is returned AS FLOWN.  What
 * mpcx_avoidance_refine is to the distance-based manoeuvres.  Arguments: those of mpcx_avoidance_window, then prop_max_step > 0 (the
 * flight's step limit), rounds >= 0, the tracker's grid M, T0, T1 and max_shift, recov (0 / 1) and q [S] (may be NULL: 0; read only
 * with recov).  M = 0: every row keeps its given time (T0, T1, max_shift are ignored).  M >= 2: the row's time is found again in
 * every pass by mpcx_conjunction_track_traj_dev of the row AS GIVEN (column 3 of pairs, in every pass: the time is not carried from
 * pass to pass) on the pass's two trajectories over linspace(T0, T1, M); max_shift <= 0: unlimited.
 * Rows are independent.  du [n][NS][3][K] is row-private, as mpcx_avoidance_window's: every row flies its own copy of the object or
 * objects that move for it, two rows that move one satellite do not see each other.  So the call has a block form: any block of
 * rows gives the bits of the whole list.  (Inside: a virtual constellation of n NS trajectories gathered after pass 0, the list
 * re-indexed to (r NS, r NS + 1), against a catalogue to (r, j).  Only rows that passed pass 0 are gathered.)
 * Passes t = 0 .. rounds + 1, a fixed number, all on one stream, nothing read back in between.
 *   t = 0: mpcx_avoidance_window on the inputs as given; out, du, sens and status have its bits.  A row FLIES when its status is
 *     MPCX_ST_OK and its ALPHA > 0; who flies never changes.  A failed row is NaN throughout and never flies; a row at or below
 *     target_p has du = 0, does not fly, and its histories repeat pass 0's figure and the given time.
 *   t >= 1, flight: for every slot of a flying row that moves U_t = U[o] + du_t-1 and Y_t from Y[o][:, 0] by
 *     mpcx_propagate_batch_ragged_dev exactly as mpcx_avoidance_refine flies (MPCX_CTRL_SEQUENCE, Kus = n_evals = Ks[o], end_tau = 1,
 *     tf = (span[1] - span[0]) / units[1], max_step = prop_max_step, columns past Ks[o] zero), under `flags`, the model of the flight
 *     and of the linearisation.  A slot that does not move keeps the given trajectory.
 *   t >= 1, time: t_t, the given time (M = 0) or the tracker's.
 *   t >= 1, covariances: recov = 0: P and cat_P as given.  recov = 1: every moving slot's covariance is mpcx_covariance_batch's chain
 *     about (Y_t, U_t) from P[o][0] and q[o], over the pass's own stage records (the last pass linearises for this alone).
 *   t >= 1, figure: Q_t = START + ENTRIES of mpcx_collision_probability_window for (i, j, ., t_t), the row's half_window and
 *     panels, on the pass's trajectories and covariances: the bits the public call returns for that data.
 *   1 <= t <= rounds, solve: |ln(Q_t / target_p)| <= tol accepts du_t-1 unchanged with 0 evaluations.  Otherwise g =
 *     mpcx_collision_window_sensitivity's sens about (Y_t, U_t) (its bits), the unit direction e_m and Gamma_t formed from g exactly
 *     as mpcx_avoidance_window forms them (the mass row Y_t's), c0 = -sum g_m du_t-1,m summed in the order slot, node, component.
 *     The unknown is the TOTAL change from the given U, du(alpha) = alpha e: the least-effort change on the linearised constraint with
 *     the effort measured from the given plan.  Two forward chains over the pass's records give X_e, the response to e, and X_prev,
 *     the response to du_t-1; Q_t(alpha) is mpcx_avoidance_window's rule with the mean moved by sgn (alpha X_e - X_prev), on the
 *     pass's frames and covariances.  alpha_1 = (c0 + Q_t ln(Q_t / target_p)) / Gamma_t (with du_t-1 = 0 pass 0's formula); Gamma_t
 *     not positive and finite: MPCX_ST_SINGULAR; alpha_1 not positive and finite: MPCX_ST_NUMERIC.  On f = ln Q_t(alpha) - ln
 *     target_p: stop at the first |f| <= tol; f(alpha_1) > 0: double alpha until f <= 0; f(alpha_1) < 0: halve alpha until f > 0;
 *     then the bracket is closed by pass 0's Illinois rule.  At most max_eval evaluations per pass: none left while bracketing
 *     MPCX_ST_INFEASIBLE, while closing MPCX_ST_MAXITER; an evaluation that is not finite MPCX_ST_NUMERIC.
 *   t = rounds + 1: flight, time, covariances and figure only.
 * A failure at t >= 1 -- the flight's status, the discretiser's, a lost event (+inf, NaN from the tracker: MPCX_ST_BADK), the
 * figure's or a solve's status -- FREEZES the row: it keeps du_t-1, reports the status in `status`, is not solved again, keeps
 * flying du_t-1, and its histories continue.
 * Outputs.  out [n][MPCX_NAW]: P0 is pass 0's Q; P1, ALPHA and DQ_LINEAR = c0 - alpha Gamma_t of the last accepted solve (a pass
 * accepted with 0 evaluations sets P1 = Q_t alone); DV_* and UMAX_* of the total du; EVALS summed over the passes.  du: the total
 * change.  status [n].  rounds_done [n]: the last pass whose solve was accepted (-1: none, or the row does not fly).  Y_out
 * [n][NS][7][K]: the last flight; a slot that does not move is a copy of the given trajectory.  P_out [n][NS][K][6][6] (may be NULL;
 * written with recov).  hist_p, hist_t [rounds + 2][n]: Q_t and t_t (pass 0: Q(0), the given time).  hist_pred [rounds + 1][n]: each
 * solve's P1, NaN where nothing was solved.  sens (may be NULL): of the last pass that linearised for a solve.
 * Argument errors: mpcx_avoidance_window's, and rounds < 0, prop_max_step <= 0, M = 1, M < 0, T1 <= T0 or a NaN max_shift with
 * M >= 2, recov outside 0 / 1, a missing required output (P_out and sens alone may be NULL): MPCX_E_BADARG, nothing enqueued.
 * The _dev variant takes device pointers throughout and a workspace of mpcx_avoidance_window_refine_workspace_bytes(n, S, K, D, M,
 * panels) bytes (D = 0 without a catalogue; 0 for n < 1, S < 1, K < 2, D < 0, M = 1, M < 0 or panels outside 1 ..
 * MPCX_PW_MAX_PANELS).  One wave per row, no atomics, every sum in a fixed order: results do not depend on the launch shape, on the
 * block of rows a row is computed in, on which optional outputs are asked for, or on the device count.
 * Not done here: these rows do not enter mpcx_avoidance_joint (two rows of one satellite get two manoeuvres), and the row's time is
 * not carried from pass to pass.
 */
size_t mpcx_avoidance_window_refine_workspace_bytes(int n, int S, int K, int D, int M, int panels);
int mpcx_avoidance_window_refine(mpcx_ctx *ctx, int n, const double *pairs, int S, int K, const int32_t *Ks, const double *Y,
                                 const double *U, const double *units, const double *span, const double *consts, int flags,
                                 double max_step, const double *P, const double *radius, int D, int cat_K, const int32_t *cat_Ks,
                                 const double *cat_Y, const double *cat_units, const double *cat_span, const double *cat_P,
                                 const double *cat_radius, double mu, const double *half_window, int panels, int who, double target_p,
                                 double tol, int max_eval, double prop_max_step, int rounds, int M, double T0, double T1,
                                 double max_shift, int recov, const double *q, double *out, double *du, double *sens, int32_t *status,
                                 int32_t *rounds_done, double *Y_out, double *P_out, double *hist_p, double *hist_t, double *hist_pred);
int mpcx_avoidance_window_refine_dev(mpcx_ctx *ctx, int n, const double *pairs, int S, int K, const int32_t *Ks, const double *Y,
                                     const double *U, const double *units, const double *span, const double *consts, int flags,
                                     double max_step, const double *P, const double *radius, int D, int cat_K, const int32_t *cat_Ks,
                                     const double *cat_Y, const double *cat_units, const double *cat_span, const double *cat_P,
                                     const double *cat_radius, double mu, const double *half_window, int panels, int who,
                                     double target_p, double tol, int max_eval, double prop_max_step, int rounds, int M, double T0,
                                     double T1, double max_shift, int recov, const double *q, double *out, double *du, double *sens,
                                     int32_t *status, int32_t *rounds_done, double *Y_out, double *P_out, double *hist_p,
                                     double *hist_t, double *hist_pred, void *workspace, void *stream);

/*
 * Joint avoidance: all of a satellite's encounters under its thrust limit.  mpcx_avoidance answers every pair on its own; it does
 * not know u_max, the plan's end state or the other pairs of the same satellite.  This call solves, for every satellite that has
 * listed encounters, one small strictly convex problem built from the same sensitivities: one thrust change that opens all of the
 * satellite's encounters at once, stays inside its thrust ball at every node and, optionally, leaves the plan's terminal position
 * and velocity where they were to first order ("avoid and return").  Nothing in the reference does this.
 *
 * Inputs.  pairs [n][4], the row side S, K, Ks, Y, U, units, span, consts, flags, max_step, P, the column side D .. cat_P, mu and
 * target exactly as mpcx_avoidance takes them, and the same single linearisation per call for all S satellites.  mover [n] int32:
 * 0 object i of the row moves, 1 object j (NULL: all 0); every pair has exactly one mover.  With a catalogue 1 is MPCX_E_BADARG
 * (the _dev variant cannot read the list on the host: such a row, or any other value, gets MPCX_ST_BADK and belongs to nobody).
 * u_max [S] the thrust limit per satellite in the plan's normalised units (NULL, or +inf for a satellite: no ball).
 * hold_terminal != 0: the terminal rows below.  tol > 0 (the wrappers' default is 1e-10), max_iter >= 1 (default 50).
 * sat0, nsat: the block of satellites sat0 .. sat0 + nsat - 1 this call computes, as the screens take row0, nrows; all arrays keep
 * their full shapes, the call writes the block's satellites and the rows of the list they own (a row whose mover is no satellite
 * 0 .. S-1 is written by the call whose block starts at satellite 0) and leaves every other element alone.
 *
 * The problem of satellite s.  Its rows are the pairs it moves for, in ascending order of their position in the list, r of them;
 * ns = Ks[s] nodes; unknowns du_m in R^3, m = 0 .. ns-1, in the plan's normalised thrust units, tf fixed.
 *   minimise 1/2 sum_m D_m |du_m|^2,  D_m = w_m c_m^2 with w_m, c_m of mpcx_avoidance (the effort integral of |da|^2 dt, trapezoid rule)
 *   (1) for each row p: sum_m a_p,m . du_m >= b_p.  Frame e_w, e_1, e_2, the miss m = (|m|, 0), W and g_m are mpcx_avoidance's, in
 *       its operation order, for the one object that moves; q = W (1, 0)^T / sqrt(W11), d0 = |m| sqrt(W11),
 *       a_p,m = q_1 g_m[0, :] + q_2 g_m[1, :], b_p = target - d0.  Without covariances (W = I) a_p,m = g_m[0, :] with the bits of
 *       mpcx_avoidance's sens.  This is the tangent half-plane of the target ellipse: by Cauchy-Schwarz in the W metric
 *       q^T (m + dm) >= target implies sqrt((m + dm)^T W (m + dm)) >= target, so a met row is never short of the target to first
 *       order.  Rows already at or beyond the target stay in the problem (b_p <= 0): another row's manoeuvre must not close them.
 *   (2) |ubar_m + du_m| <= u_max[s] at every node, ubar = U[s].
 *   (3) hold_terminal: sum_m T_m du_m = 0, T_m (6 x 3) the derivative of the last node's normalised position and velocity with
 *       respect to u_m: the adjoint recursion of mpcx_avoidance seeded with [I_6 | 0] at node ns - 1 and swept over the whole
 *       horizon (lam_ns-1 = [I_6 | 0], lam_m = lam_m+1 A_m, T_m = lam_m+1 B_kn[m] (m <= ns-2) + lam_m B_kp[m-1] (m >= 1)).
 * Method.  Multipliers z = (y in R^6 free, lambda in R^r >= 0); an encounter row is taken in units of the target (a / target,
 * b / target, lambda * target), the terminal rows as they are.  du_m(z) = proj_ball(ubar_m + (A^T z)_m / D_m) - ubar_m in closed
 * form per node; F(z) = [T du(z); min(c_p lambda_p, (a_p du(z) - b_p) / target)] = 0 is solved from z = 0 by a semismooth Newton
 * iteration.  c_p = sum_m |a_p,m / target|^2 / D_m is the row's own authority, what a multiplier of 1 moves the row by when it acts
 * alone: it brings multiplier and slack to one scale, whatever the units of the target (with the bare min(lambda, slack) a row whose
 * multiplier must come back from 1e5 to 0 never passes the step control).
 * Row p is active when c_p lambda_p > its slack.  H = sum_m A_m J_m A_m^T / D_m with J_m the projection's Jacobian (the nodes in
 * ascending order).  On the active rows H dz = -F + H[., inactive] lambda, on the inactive ones dz = -lambda.  Cholesky of the
 * active block; a pivot at or below 1e-12 of its own diagonal entry is "not positive definite".  z + t dz with t = 1, 1/2, ... (30
 * halvings at most) until max |F| falls or is <= tol.  Converged: max |F| <= tol, every inactive row's lambda exactly 0, no lambda
 * negative.
 *
 * Outputs.  du [S][3][K]: the thrust change; zero for a satellite without rows and for nodes past ns.  sat_out [S][MPCX_NAJ]
 * (MPCX_AJ_*), all zero for a satellite without rows.  row_out [n][MPCX_NAR] (MPCX_AR_*): D0 comes from the pair alone; the other
 * four are NaN unless the owning satellite's status is OK.  rows [n][3][K] (may be NULL): the a_p, zero past the row's node k + 1.
 * tsens [S][6][3][K] (may be NULL): the T_m, zero past ns, all zero for a satellite whose problem was not set up (no rows, a failed
 * row, too many rows) or without hold_terminal.  Results have the same bits with and without rows and tsens.
 * row_status [n]: mpcx_avoidance's per-pair statuses (BADK, NUMERIC, the discretiser's; there is no per-pair SINGULAR here), BADK
 * for a bad mover.  A failed row is NaN in row_out and rows.  sat_status [S]: the first status that is not OK among the
 * satellite's rows in list order; else MPCX_ST_BADK with more than MPCX_AJ_MAX_ROWS rows; else MPCX_ST_INFEASIBLE when the ball
 * alone forbids a row, sum_m (u_max |a_p,m| - a_p,m . ubar_m) < b_p, tested before the first iteration; else MPCX_ST_SINGULAR when
 * the Newton matrix on the active rows is not positive definite (dependent rows -- two identical active rows are SINGULAR, they do
 * not share a multiplier --, an active encounter at the first node, 3 ns < 6 + r); else MPCX_ST_MAXITER without convergence within
 * max_iter, when no step length reduces max |F|, or on a non-finite iterate.  A satellite whose status is not OK is NaN in du and
 * sat_out; the other satellites are untouched by it.  A satellite without rows has status OK.
 * n < 1, S < 1, K < 2, mu <= 0, target or tol not positive and finite, max_iter < 1, a block outside 0 .. S-1 or nsat < 1,
 * max_step <= 0, a bad flag (as mpcx_avoidance), P without cat_P or the reverse with a catalogue, a bad mover (host variant):
 * MPCX_E_BADARG, nothing enqueued.
 * The _dev variant takes device pointers throughout and a workspace of mpcx_avoidance_joint_workspace_bytes(n, S, K) bytes (stage
 * records, tf, the discretiser's status, the g_m, the rows when rows is NULL, per-pair scalars and owners, the T_m when tsens is
 * NULL, the projection's Jacobians; 0 for n < 1, S < 1 or K < 2; contents unspecified on entry and exit).  The g_m and the rows are
 * 12 n K doubles: 630 MB at n = 65 536, K = 100 -- a list that long is better given in blocks of pairs per satellite block.  One wave per pair, one
 * wave per satellite; every sum runs in ascending index order or in a fixed butterfly and nothing crosses a workgroup: results do
 * not depend on the launch shape, on the block of satellites, on the device count, or on pairs that belong to other satellites.
 */
#define MPCX_AJ_MAX_ROWS 8
enum { MPCX_AJ_COST = 0,    /* 1/2 sum_m D_m |du_m|^2, (m/s^2)^2 s */
       MPCX_AJ_DV,          /* sum_m w_m |da_m|, m/s */
       MPCX_AJ_UMAX,        /* max_m |ubar_m + du_m|, normalised */
       MPCX_AJ_ROWS,        /* r: the satellite's rows */
       MPCX_AJ_ACTIVE,      /* rows with lambda > 0 */
       MPCX_AJ_ONBALL,      /* nodes the ball projects */
       MPCX_AJ_ITERS,       /* Newton iterations */
       MPCX_AJ_RESIDUAL,    /* final max |F| (encounter rows in units of the target) */
       MPCX_NAJ };
enum { MPCX_AR_D0 = 0,      /* d0: the distance now, in the target's metric */
       MPCX_AR_MARGIN,      /* the linear margin q^T (m + dm) = d0 + sum_m a_p,m . du_m, to compare with target */
       MPCX_AR_DIST,        /* the predicted distance sqrt((m + dm)^T W (m + dm)), dm = sum_m g_m[0:2] du_m */
       MPCX_AR_LAMBDA,      /* the row's multiplier, in the row's own units (effort per unit of the target's metric) */
       MPCX_AR_DT,          /* shift of the time of closest approach, -(e_w row of sum_m g_m du_m) / |w|, s */
       MPCX_NAR };
size_t mpcx_avoidance_joint_workspace_bytes(int n, int S, int K);
int mpcx_avoidance_joint(mpcx_ctx *ctx, int n, const double *pairs, const int32_t *mover, int S, int K, const int32_t *Ks,
                         const double *Y, const double *U, const double *units, const double *span, const double *consts, int flags,
                         double max_step, const double *P, int D, int cat_K, const int32_t *cat_Ks, const double *cat_Y,
                         const double *cat_units, const double *cat_span, const double *cat_P, double mu, double target,
                         const double *u_max, int hold_terminal, double tol, int max_iter, int sat0, int nsat, double *du,
                         double *sat_out, double *row_out, double *rows, double *tsens, int32_t *sat_status, int32_t *row_status);
int mpcx_avoidance_joint_dev(mpcx_ctx *ctx, int n, const double *pairs, const int32_t *mover, int S, int K, const int32_t *Ks,
                             const double *Y, const double *U, const double *units, const double *span, const double *consts,
                             int flags, double max_step, const double *P, int D, int cat_K, const int32_t *cat_Ks,
                             const double *cat_Y, const double *cat_units, const double *cat_span, const double *cat_P, double mu,
                             double target, const double *u_max, int hold_terminal, double tol, int max_iter, int sat0, int nsat,
                             double *du, double *sat_out, double *row_out, double *rows, double *tsens, int32_t *sat_status,
                             int32_t *row_status, void *workspace, void *stream);

/*
 * Iterated avoidance: the manoeuvre flown again, looked at again and corrected, on the device.  mpcx_avoidance_joint stops at a
 * first-order answer that nothing flies: flown through the nonlinear dynamics it falls short of the target by some 1e-3 of it, the
 * held end state drifts, and a row whose other object is moved by another row (the wrappers' `coupled`) is not corrected at all.
 * This call closes the loop for the whole list and all S satellites on one device -- a coupled row needs every mover's new
 * trajectory in every round, so there is no block form (no sat0, nsat).
 *
 * Inputs.  Everything mpcx_avoidance_joint takes except sat0 and nsat; `flags` is the model of the flight AND of the linearisation.
 * M, T0, T1: the re-screen's grid linspace(T0, T1, M), as mpcx_conjunction_pairs_traj takes it.  prop_max_step > 0: the flight's
 * step limit.  rounds >= 0: the number of corrections.  P and cat_P stay as given over all passes.
 *
 * Passes t = 0 .. rounds + 1.
 *   t = 0: mpcx_avoidance_joint on (pairs, Y, U) as given; du, sat_out, row_out, rows, tsens and the statuses have its bits.  A
 *     satellite FLIES when this pass gave it rows and status MPCX_ST_OK (a finite du); who flies never changes afterwards.
 *   t >= 1, the flight: U_t = U + du_t-1 for a satellite that flies, U otherwise.  Y_t[s] of a satellite that flies is
 *     mpcx_propagate_batch_ragged_dev from Y[s][:, 0] over tf = (span[1] - span[0]) / units[1] under MPCX_CTRL_SEQUENCE with the table
 *     U_t[s], Kus = n_evals = Ks, end_tau = 1, max_step = prop_max_step (columns past Ks[s] zero); every other satellite keeps Y[s].
 *   t >= 1, the re-screen: mpcx_conjunction_pairs_traj_dev of the given list on Y_t (and the catalogue); its out [n][4] IS this
 *     pass's list.  A row without a valid interval (+inf, NaN) gets the status the joint call gives a row with that time.
 *   t >= 1, the solve: one linearisation about (Y_t, U_t), the rows of the joint call, and per satellite the joint call's problem
 *     with three changes.  The unknown du is the TOTAL change from the given U (the centre of the ball projection and the origin the
 *     effort is measured from: du_m(z) = proj_ball(U_m + (A^T z)_m / D_m) - U_m, and MPCX_AJ_UMAX, _COST, _DV are of U + du and du);
 *     row p reads sum_m a_p,m . du_m >= b_p + sum_m a_p,m . (U_t,m - U_m), the ball-alone INFEASIBLE test uses that value and U; the
 *     terminal rows read sum_m T_m du_m = sum_m T_m du_t-1,m - (Y_t[0:6, ns-1] - Y[0:6, ns-1]) -- the end state is held to the GIVEN
 *     plan's; the iteration starts from the z of the satellite's last converged solve instead of 0 (a cold start of a later round does
 *     not converge in general).  D_m takes the mass row of Y_t.  row_out's MARGIN, DIST and DT are predictions from this pass's
 *     linearisation for the change U + du - U_t.
 *   t = rounds + 1: the flight, the re-screen and the rows' d0, no solve: every call returns its answer AS FLOWN.
 * Failures.  Pass 0's result is taken as it is: NaN on failure; such a satellite never flies and counts as not moving.  For t >= 1 a
 * solve that fails (any status of the joint call) or a flight that fails (the rollout's status; its Y_t is the given Y[s]) keeps
 * du_t-1, sat_out and the satellite's rows of row_out as they were, reports its status in sat_status and FREEZES the satellite: no
 * more solves, and it keeps flying du_t-1.  rounds_done [S]: the index of the last pass whose solve was accepted (-1: none, or no rows).
 *
 * Outputs.  The joint call's: du [S][3][K] the total change from U, sat_out and row_out of the last accepted solve, sat_status,
 * row_status; rows [n][3][K] and tsens [S][6][3][K] (each may be NULL) of the last pass that solved (pass `rounds`; a satellite left
 * alone by it keeps what an earlier pass wrote).  Y_out [S][7][K]: the last flight.  pairs_out [n][4]: the last re-screen.
 * hist_d0, hist_tca [rounds + 2][n]: each pass's d0 in the target's metric and the time the row was
 * taken at (pass 0: column 3 of pairs; later: the re-screen's).  hist_term [rounds + 2][S]: max |Y_t[0:6, ns-1] - Y[0:6, ns-1]|,
 * normalised; 0 for a satellite that does not fly and in pass 0.  rhs_rows [n], rhs_term [S][6] (each may be NULL): the right-hand
 * sides of pass `rounds`'s solve in the rows' own units (NaN / 0 for rows and satellites that pass left alone).
 * Every sum keeps a fixed order; results do not depend on the launch shape or on which optional outputs are asked for.
 * Argument errors are the joint call's, plus rounds < 0, M < 2, T1 <= T0, prop_max_step <= 0, a missing required output:
 * MPCX_E_BADARG, nothing enqueued.  The _dev variant takes device pointers throughout and a workspace of
 * mpcx_avoidance_refine_workspace_bytes(n, S, K, D, M) bytes (D = 0 without a catalogue; 0 for n < 1, S < 1, K < 2, D < 0 or M < 2;
 * contents unspecified on entry and exit); it enqueues everything on `stream`, the number of passes is fixed and nothing is read back
 * or waited for between them.
 */
size_t mpcx_avoidance_refine_workspace_bytes(int n, int S, int K, int D, int M);
int mpcx_avoidance_refine(mpcx_ctx *ctx, int n, const double *pairs, const int32_t *mover, int S, int K, const int32_t *Ks,
                          const double *Y, const double *U, const double *units, const double *span, const double *consts, int flags,
                          double max_step, const double *P, int D, int cat_K, const int32_t *cat_Ks, const double *cat_Y,
                          const double *cat_units, const double *cat_span, const double *cat_P, double mu, double target,
                          const double *u_max, int hold_terminal, double tol, int max_iter, int M, double T0, double T1,
                          double prop_max_step, int rounds, double *du, double *sat_out, double *row_out, double *rows, double *tsens,
                          int32_t *sat_status, int32_t *row_status, double *Y_out, double *pairs_out, double *hist_d0,
                          double *hist_tca, double *hist_term, int32_t *rounds_done, double *rhs_rows, double *rhs_term);
int mpcx_avoidance_refine_dev(mpcx_ctx *ctx, int n, const double *pairs, const int32_t *mover, int S, int K, const int32_t *Ks,
                              const double *Y, const double *U, const double *units, const double *span, const double *consts,
                              int flags, double max_step, const double *P, int D, int cat_K, const int32_t *cat_Ks,
                              const double *cat_Y, const double *cat_units, const double *cat_span, const double *cat_P, double mu,
                              double target, const double *u_max, int hold_terminal, double tol, int max_iter, int M, double T0,
                              double T1, double prop_max_step, int rounds, double *du, double *sat_out, double *row_out, double *rows,
                              double *tsens, int32_t *sat_status, int32_t *row_status, double *Y_out, double *pairs_out,
                              double *hist_d0, double *hist_tca, double *hist_term, int32_t *rounds_done, double *rhs_rows,
                              double *rhs_term, void *workspace, void *stream);

/*
 * mpcx_avoidance_refine_tracked: mpcx_avoidance_refine for a list that holds SEVERAL encounters of one pair (the rows of
 * mpcx_conjunction_events).  With mpcx_conjunction_pairs_traj_dev as the re-screen every row of a pair carries the pair's global
 * minimum from pass 1 on: two identical rows make the solve singular (MPCX_ST_SINGULAR) under the hold, and without it the second
 * encounter is never looked at again.  Here the re-screen of every pass t >= 1 is mpcx_conjunction_track_traj_dev of the GIVEN list
 * on Y_t with this call's max_shift (info NULL): each row follows the event nearest the time it was given, column 3 of `pairs`, in
 * every pass -- not the time the pass before found.  Everything else is mpcx_avoidance_refine word for word: the arguments (plus
 * max_shift after rounds), the passes, the outputs, the workspace and its size, the failures.  On a list whose every row is its
 * pair's only event within reach both calls return the same bits.
 * A row that loses its event -- none on Y_t, or none within max_shift -- is (+inf, NaN) in that pass's list, exactly the row
 * without a valid interval of mpcx_avoidance_refine: the joint call gives a row with a NaN time MPCX_ST_BADK, so the pass's solve
 * of the satellite that moves for it fails with that status, the satellite keeps du_t-1, reports MPCX_ST_BADK in sat_status and is
 * frozen (no more solves, it keeps flying du_t-1); hist_d0 and hist_tca of the row are NaN in that pass.
 * A NaN max_shift is MPCX_E_BADARG; max_shift <= 0 is unlimited.
 */
int mpcx_avoidance_refine_tracked(mpcx_ctx *ctx, int n, const double *pairs, const int32_t *mover, int S, int K, const int32_t *Ks,
                                  const double *Y, const double *U, const double *units, const double *span, const double *consts,
                                  int flags, double max_step, const double *P, int D, int cat_K, const int32_t *cat_Ks,
                                  const double *cat_Y, const double *cat_units, const double *cat_span, const double *cat_P, double mu,
                                  double target, const double *u_max, int hold_terminal, double tol, int max_iter, int M, double T0,
                                  double T1, double prop_max_step, int rounds, double max_shift, double *du, double *sat_out,
                                  double *row_out, double *rows, double *tsens, int32_t *sat_status, int32_t *row_status, double *Y_out,
                                  double *pairs_out, double *hist_d0, double *hist_tca, double *hist_term, int32_t *rounds_done,
                                  double *rhs_rows, double *rhs_term);
int mpcx_avoidance_refine_tracked_dev(mpcx_ctx *ctx, int n, const double *pairs, const int32_t *mover, int S, int K, const int32_t *Ks,
                                      const double *Y, const double *U, const double *units, const double *span, const double *consts,
                                      int flags, double max_step, const double *P, int D, int cat_K, const int32_t *cat_Ks,
                                      const double *cat_Y, const double *cat_units, const double *cat_span, const double *cat_P,
                                      double mu, double target, const double *u_max, int hold_terminal, double tol, int max_iter, int M,
                                      double T0, double T1, double prop_max_step, int rounds, double max_shift, double *du,
                                      double *sat_out, double *row_out, double *rows, double *tsens, int32_t *sat_status,
                                      int32_t *row_status, double *Y_out, double *pairs_out, double *hist_d0, double *hist_tca,
                                      double *hist_term, int32_t *rounds_done, double *rhs_rows, double *rhs_term, void *workspace,
                                      void *stream);

/*
 * mpcx_collision_probability_mc: the collision probability of listed rows by sampled flights through the truth model.  Every other
 * probability of this library is a linearised Gaussian figure (chained transition matrices, a fixed quadrature rule); here n_samples
 * worlds are drawn -- initial states, masses, thrust execution errors --, every object of every row is flown through the nonlinear
 * dynamics by mpcx_propagate_batch_ragged_dev, and what is counted is how often the two flown objects come within R = radius_i +
 * radius_j inside the row's window.  There is no white process noise: the figure corresponds to mpcx_covariance_batch /
 * mpcx_covariance_thrust_batch with q = 0.  There is no mu argument: the flight takes mu from consts.
 * Arguments.  n, pairs [n][4] rows exactly as the screens and mpcx_conjunction_events write them.  The row side: S, K, Ks, Y [S][7][K],
 * U [S][3][K] (NULL: zero thrust), units, span, consts, flags as mpcx_covariance_batch takes them; prop_max_step > 0 the flight's
 * step limit; P0 [S][6][6] in m and m/s at the FIRST node (its upper triangle is read); exec [S][MPCX_NEXEC] (NULL: perfect
 * execution) and m_var0 [S] (NULL: 0) with mpcx_covariance_thrust_batch's meaning; radius [S].  The column side: D, cat_K, cat_Ks,
 * cat_Y, cat_units, cat_span, cat_consts, cat_P0, cat_radius; cat_Y = NULL: the all-pairs form (j indexes the constellation, the
 * other cat_ arguments are ignored); catalogue objects fly with zero thrust and no execution error under the same flags.
 * half_window [n] in seconds; scan >= 1 scan intervals per window; n_samples >= 1; seed; max_flights: 0 the library's default
 * (262144), otherwise an upper bound on the virtual trajectories of one side in flight at once, which bounds the workspace: samples
 * are processed in chunks of floor(max_flights / (n NS)) samples, at least one per chunk (NS = 2 in the all-pairs form, 1 with a
 * catalogue, whose side flies as many again).  The chunking changes no bit.
 * One sample s is one world.  Every draw is Philox4x32-10 (ten rounds, multipliers D2511F53 / CD9E8D57, Weyl constants 9E3779B9 /
 * BB67AE85) with key = (seed low word, seed high word) and counter = (s, object index, block, side), side 0 the constellation and 1
 * the catalogue: the draws of object o in sample s do not depend on the list, the row, the chunking, the launch shape or the device,
 * so a satellite that appears in several rows has the SAME flown trajectory in all of them, any block of rows gives the bits of
 * the whole list, and the per-sample records of different rows are joint samples.  One block gives two uniforms, u = ((w_a >> 5) 2^26
 * + (w_b >> 6) + 0.5) 2^-53 from the words (0, 1) and (2, 3) -- strictly inside (0, 1): in binary64 the + 0.5 is rounded to even above
 * 2^52, and the one value midway between 1 - 2^-53 and 1 (all 53 bits set) is rounded down --
 * and from them two normals, z_a = r cos(2 pi u_2), z_b = r sin(2 pi u_2), r = sqrt(-2 ln u_1).  Blocks 0-2:
 * the six state normals z_0 .. z_5 (block b gives z_2b, z_2b+1); block 3: the mass normal (z_a); blocks 4 + 2k and 5 + 2k: the
 * normals of thrust node k (z_1 = z_a, z_2 = z_b of the first, z_3 = z_a of the second).
 *   initial state   x0 = Y[o][0:6, 0] + D^-1 L z, D = diag(L, L, L, V, V, V) the units, P0 = L L^T by columns for a positive
 *                   SEMI-definite P0.  The zero-pivot rule: with d_j = P0_jj - sum_k<j L_jk^2, c_ij = P0_ji - sum_k<j L_ik L_jk and
 *                   tol_j = 1e-12 P0_jj: d_j > tol_j is a regular pivot (L_jj = sqrt d_j, L_ij = c_ij / L_jj); |d_j| <= tol_j is a zero
 *                   pivot, column j of L is zero and every c_ij^2 <= tol_j P0_ii is required; anything else -- d_j < -tol_j, a
 *                   negative or non-finite diagonal entry -- cannot be factored: MPCX_ST_NUMERIC
 *   mass            m0 = Y[o][6, 0] + sqrt(m_var0) z
 *   thrust node k   u_k + s_par z_1 u^ + s_perp (z_2 e_1 + z_3 e_2), s_par, s_perp and u_off as in mpcx_covariance_thrust_batch, e_1 the
 *                   coordinate axis on which |u^| is smallest (the first of equal ones) made orthogonal to u^ and normalised, e_2 = u^
 *                   x e_1; nothing is added at a node with |u_k| <= u_off, and no draw is made there.
 * Flight.  Every (row, slot, sample) is a virtual satellite flown by mpcx_propagate_batch_ragged_dev exactly as
 * mpcx_avoidance_window_refine flies: MPCX_CTRL_SEQUENCE on the sample's thrust table (a zero table for U = NULL and for the
 * catalogue), Kus = n_evals = Ks[o], end_tau = 1, tf = (span[1] - span[0]) / units[1], the given flags, prop_max_step.
 * Scan, per (row, sample).  The window [t_a, t_b] is mpcx_collision_probability_window's: t +- half_window cut to both spans, with
 * the same MPCX_ST_BADK tests (made on the given trajectories).  It is cut into `scan` equal intervals, instant i at t_a + i (t_b -
 * t_a) / scan, the last one at t_b.  Both objects' positions and velocities at the instants come from mpcx_ephemeris_batch's cubic
 * Hermite on their own FLOWN nodes; inside an interval the relative position is the cubic Hermite of the end differences and end
 * relative velocities, and its minimum follows the screens' interval rule: the ends, the clamped minimum of the chord, three Newton
 * steps.  With q0, q1, qmin the squared distances at an interval's ends and at its minimum: inside_start = q(t_a) <= R^2; an
 * interval counts one ENTRY when q0 > R^2 and (q1 <= R^2 or qmin <= R^2); entries is their number; hit = inside_start or entries >= 1;
 * (dmin, t_min) the smallest distance found and its time, the earliest of equal ones.  Two entries inside one scan interval count
 * as one, and an exit and re-entry inside an interval that starts inside counts as none: that is the resolution `scan` must buy.
 * Outputs.  counts [n][MPCX_NMCC] int64 (MPCX_MCC_*): integers, independent of any summation order.  out [n][MPCX_NMC] (MPCX_MC_*),
 * formed on the device from the counts with N = N_OK = flown - failed:  P_HIT = hits / N;  SE_HIT = sqrt(P_HIT (1 - P_HIT) / N);
 * START, ENTRIES the means per sample;  SE_BOUND = sqrt(var / N), var = (sum b^2 - (sum b)^2 / N) / (N - 1) the sample variance of
 * b = inside_start + entries (0 for N = 1);  EXCESS = START + ENTRIES - P_HIT, how far the window rule's figure lies above the
 * probability because paths re-enter;  TA, TB, N_OK.  status [n].  Optional, NULL allowed, and asking for them changes no other bit:
 * samples [n][n_samples][MPCX_NMS] (MPCX_MS_*), Y_samples [n][NS][n_samples][7][K] and U_samples [n][NS][n_samples][3][K], the row
 * side's flown trajectories and executed thrust tables (slot 0 = i, 1 = j; columns past Ks come back zero; a failed flight is NaN in
 * Y_samples).
 * status: the window call's statuses; then MPCX_ST_BADK for an object whose span and time unit give no positive finite tf;
 * then MPCX_ST_NUMERIC for a P0 that cannot be factored, or a negative or non-finite exec entry or m_var0, of either object; then
 * MPCX_ST_NUMERIC for a row of which no sample survived its flight.  A sample whose flight of either object ends with a status other
 * than 0 (or without a finite distance: MPCX_ST_NUMERIC) is counted in FAILED and left out of every other count; its samples row is
 * NaN, NaN, 0, 0, the status.  A failed row is NaN in out (and in samples' distances and Y_samples / U_samples), zero in counts, and
 * leaves its neighbours alone.  R <= 0: zeros in out but TA, TB, zeros in counts and samples, MPCX_ST_OK, as in the window call.
 * n < 1, S < 1, K < 2, prop_max_step <= 0, an unknown flag, MPCX_FLAG_ATMO without drag or without an atmosphere on the context, scan <
 * 1, n_samples < 1, max_flights < 0, a catalogue with D < 1 or cat_K < 2 or without one of its arrays, a NULL pairs, Y, units, span,
 * consts, P0, radius, half_window, counts, out or status: MPCX_E_BADARG with "collision_probability_mc" in the message, nothing
 * enqueued.  The _dev variant takes device pointers throughout and a workspace of mpcx_collision_probability_mc_workspace_bytes(n,
 * S, K, D, cat_K, n_samples, max_flights) bytes (D = 0: the all-pairs form; 0 for arguments the call would refuse; contents
 * unspecified on entry and exit).  All passes are enqueued on one stream, their number is fixed by the arguments, nothing is read
 * back; the counts are summed with 64-bit integer atomics.
 */
#define MPCX_NMCC 6
enum { MPCX_MCC_FLOWN = 0,  /* samples flown */
       MPCX_MCC_FAILED,     /* of them: a flight status other than 0 */
       MPCX_MCC_START,      /* sum inside_start */
       MPCX_MCC_ENTRIES,    /* sum entries */
       MPCX_MCC_SQUARES,    /* sum (inside_start + entries)^2 */
       MPCX_MCC_HIT };      /* sum hit */
#define MPCX_NMC 9
enum { MPCX_MC_P_HIT = 0, MPCX_MC_SE_HIT, MPCX_MC_START, MPCX_MC_ENTRIES, MPCX_MC_SE_BOUND, MPCX_MC_EXCESS, MPCX_MC_TA, MPCX_MC_TB,
       MPCX_MC_N_OK };
#define MPCX_NMS 5
enum { MPCX_MS_DMIN = 0,    /* m */
       MPCX_MS_T_MIN,       /* s */
       MPCX_MS_INSIDE_START, MPCX_MS_ENTRIES,
       MPCX_MS_STATUS };    /* the flight's MPCX_ST_* (slot 0's first, then the column object's) */
size_t mpcx_collision_probability_mc_workspace_bytes(int n, int S, int K, int D, int cat_K, int n_samples, int max_flights);
int mpcx_collision_probability_mc(mpcx_ctx *ctx, int n, const double *pairs, int S, int K, const int32_t *Ks, const double *Y,
                                  const double *U, const double *units, const double *span, const double *consts, int flags,
                                  double prop_max_step, const double *P0, const double *exec, const double *m_var0, const double *radius,
                                  int D, int cat_K, const int32_t *cat_Ks, const double *cat_Y, const double *cat_units,
                                  const double *cat_span, const double *cat_consts, const double *cat_P0, const double *cat_radius,
                                  const double *half_window, int scan, int n_samples, uint64_t seed, int max_flights, int64_t *counts,
                                  double *out, int32_t *status, double *samples, double *Y_samples, double *U_samples);
int mpcx_collision_probability_mc_dev(mpcx_ctx *ctx, int n, const double *pairs, int S, int K, const int32_t *Ks, const double *Y,
                                      const double *U, const double *units, const double *span, const double *consts, int flags,
                                      double prop_max_step, const double *P0, const double *exec, const double *m_var0,
                                      const double *radius, int D, int cat_K, const int32_t *cat_Ks, const double *cat_Y,
                                      const double *cat_units, const double *cat_span, const double *cat_consts, const double *cat_P0,
                                      const double *cat_radius, const double *half_window, int scan, int n_samples, uint64_t seed,
                                      int max_flights, int64_t *counts, double *out, int32_t *status, double *samples,
                                      double *Y_samples, double *U_samples, void *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MPCX_H */
