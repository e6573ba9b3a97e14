// encounter_host.hpp -- the host side of the listed-pair calls.  What is shared:
//   EncGeometry     the list and its two sides, with its argument tests (geom_check_*), its uploads (geom_upload) and the CpSide pair
//                   its kernels take (enc_sides); every call of the family is "that, plus my own few members"
//   EncProblem      the geometry plus the model of its linearisation and the target, with enc_check / enc_upload / enc_linearise:
//                   mpcx_avoidance*, mpcx_avoidance_joint*, mpcx_avoidance_refine*, mpcx_collision_window_sensitivity*,
//                   mpcx_avoidance_window*, mpcx_avoidance_window_refine*; mpcx_covariance_batch* share the linearisation
//   MPCX_GEOMETRY / MPCX_ENC_PROBLEM   an entry point's arguments, under their names in include/mpcx.h, as either
//   Carver, LinWorkspace, FlightSet    the workspace carver, the linearisation's regions, the trajectories flown again
// Results and the tail of a host form (DeviceArena::result, host_run) are mpcx_host.hpp's.  A call owns its kernel arguments, its
// own members with their tests and uploads, its workspace layout and its enqueue.
#pragma once
#include "collision_device.hpp"                                     // CpSide
#include "mpcx_host.hpp"

namespace mpcx {

// The list and its two sides as every listed-pair call takes them: the rows, the constellation with its covariances and radii, the
// catalogue (optional, with its own), mu.  A call that has no P or no radii leaves them NULL.
struct EncGeometry {
    int n;
    const double *pairs;
    int S, K;
    const int32_t *Ks;
    const double *Y, *units, *span, *P, *radius;
    int D, cat_K;
    const int32_t *cat_Ks;
    const double *cat_Y, *cat_units, *cat_span, *cat_P, *cat_radius;
    double mu;
};
// the arguments of an entry point, under their names in include/mpcx.h, as an EncGeometry (RADIUS, CAT_RADIUS: nullptr where it has none)
#define MPCX_GEOMETRY(RADIUS, CAT_RADIUS) \
    {n, pairs, S, K, Ks, Y, units, span, P, RADIUS, D, cat_K, cat_Ks, cat_Y, cat_units, cat_span, cat_P, CAT_RADIUS, mu}

inline int enc_fail(mpcx_ctx *ctx, const char *name, const char *what)
{
    char msg[256];
    snprintf(msg, sizeof msg, "%s: %s", name, what);
    return ctx_fail(ctx, MPCX_E_BADARG, msg);
}

// The argument tests of the geometry for the call `name`, in the two steps between which a call tests its own scalars: the sizes,
// then the arrays.
inline int geom_check_sizes(mpcx_ctx *ctx, const EncGeometry &g, const char *name)
{
    if (g.n < 1 || g.S < 1 || g.K < 2 || !(g.mu > 0.0)) return enc_fail(ctx, name, "need n>=1, S>=1, K>=2, mu>0");
    return MPCX_OK;
}
// a catalogue's own: own_given / names as below, for what is required with cat_Y
inline int geom_check_catalogue(mpcx_ctx *ctx, const EncGeometry &g, const char *name, bool own_given, const char *names)
{
    if (!g.cat_Y) return MPCX_OK;
    if (g.D < 1 || g.cat_K < 2) return enc_fail(ctx, name, "a catalogue needs D>=1, cat_K>=2");
    if (!g.cat_units || !g.cat_span || !own_given) {
        char what[160];
        snprintf(what, sizeof what, "%s are required with cat_Y", names);
        return enc_fail(ctx, name, what);
    }
    return MPCX_OK;
}
// full: the call requires P, radius and, with a catalogue, cat_P, cat_radius (the probability family); else all four are optional
// here (the avoidance family has no radii and takes P or not).  own_given / names: whether the call's own required arrays are all
// there, and the whole list of required arrays as the message names it.
inline int geom_check_arrays(mpcx_ctx *ctx, const EncGeometry &g, const char *name, bool full, bool own_given, const char *names)
{
    if (!g.pairs || !g.Y || !g.units || !g.span || (full && (!g.P || !g.radius)) || !own_given) {
        char what[224];
        snprintf(what, sizeof what, "%s are required", names);
        return enc_fail(ctx, name, what);
    }
    return geom_check_catalogue(ctx, g, name, !full || (g.cat_P && g.cat_radius),
                                full ? "cat_units, cat_span, cat_P and cat_radius" : "cat_units and cat_span");
}

// the geometry's host arrays replaced by copies on the device
inline void geom_upload(DeviceArena &ar, EncGeometry &g)
{
    const size_t S = (size_t)g.S, K = (size_t)g.K, D = (size_t)g.D, cK = (size_t)g.cat_K;
    g.pairs = ar.upload(g.pairs, (size_t)g.n * 4);
    g.Y = ar.upload(g.Y, S * 7 * K); g.units = ar.upload(g.units, S * 2); g.span = ar.upload(g.span, S * 2);
    g.Ks = g.Ks ? ar.upload(g.Ks, S) : nullptr;
    g.P = g.P ? ar.upload(g.P, S * K * 36) : nullptr;
    g.radius = g.radius ? ar.upload(g.radius, S) : nullptr;
    if (g.cat_Y) {
        g.cat_Y = ar.upload(g.cat_Y, D * 7 * cK); g.cat_units = ar.upload(g.cat_units, D * 2);
        g.cat_span = ar.upload(g.cat_span, D * 2);
        g.cat_P = g.cat_P ? ar.upload(g.cat_P, D * cK * 36) : nullptr;
        g.cat_radius = g.cat_radius ? ar.upload(g.cat_radius, D) : nullptr;
        g.cat_Ks = g.cat_Ks ? ar.upload(g.cat_Ks, D) : nullptr;
    }
}

// The two sides of the list as the kernels take them: the constellation, and the catalogue where there is one, else the
// constellation again.
inline void enc_sides(const EncGeometry &g, CpSide &row, CpSide &col)
{
    row = CpSide{g.S, g.K, g.Ks, g.Y, g.units, g.span, g.P, g.radius};
    col = g.cat_Y ? CpSide{g.D, g.cat_K, g.cat_Ks, g.cat_Y, g.cat_units, g.cat_span, g.cat_P, g.cat_radius} : row;
}

// a listed-pairs problem as every avoidance entry point takes it: the geometry, the plan that was screened and the model of its
// linearisation, the target
struct EncProblem : EncGeometry {
    const double *U, *consts;
    int flags;
    double max_step, target;
};
#define MPCX_ENC_PROBLEM(RADIUS, CAT_RADIUS, TARGET) {MPCX_GEOMETRY(RADIUS, CAT_RADIUS), U, consts, flags, max_step, TARGET}

// The argument tests of the call `name` that every avoidance entry point makes.  outputs_given / outputs: whether the call's own
// required output arrays are all there, and their names as the message lists them behind the inputs.
inline int enc_check(mpcx_ctx *ctx, const EncProblem &p, const char *name, bool outputs_given, const char *outputs)
{
    if (int rc = geom_check_sizes(ctx, p, name)) return rc;
    if (!(p.target > 0.0) || !(p.target < __builtin_inf())) return enc_fail(ctx, name, "target must be a positive finite number");
    if (!(p.max_step > 0.0)) return enc_fail(ctx, name, "max_step must be > 0");
    if (p.flags & ~(MPCX_FLAG_DRAG | MPCX_FLAG_J2 | MPCX_FLAG_ATMO))
        return enc_fail(ctx, name, "flags are MPCX_FLAG_DRAG | MPCX_FLAG_J2 | MPCX_FLAG_ATMO");
    char names[192];
    snprintf(names, sizeof names, "pairs, Y, U, units, span, consts, %s", outputs);
    if (int rc = geom_check_arrays(ctx, p, name, false, p.U && p.consts && outputs_given, names)) return rc;
    if (p.cat_Y && (p.P != nullptr) != (p.cat_P != nullptr))
        return enc_fail(ctx, name, "P and cat_P come together (a Mahalanobis target) or not at all (metres)");
    return ctx_check_atmosphere(ctx, p.flags, name);
}

// which object of every pair moves (host array [n] or NULL: object i)
inline int check_mover(mpcx_ctx *ctx, const EncProblem &p, const int32_t *mover, const char *name)
{
    if (mover)
        for (int r = 0; r < p.n; ++r)
            if (mover[r] < 0 || mover[r] > 1 || (p.cat_Y && mover[r] != 0))
                return enc_fail(ctx, name, "mover is 0 (object i) or 1 (object j); against a catalogue only 0");
    return MPCX_OK;
}

// the problem's host arrays replaced by copies on the device
inline void enc_upload(DeviceArena &ar, EncProblem &p)
{
    geom_upload(ar, p);
    p.U = ar.upload(p.U, (size_t)p.S * 3 * p.K); p.consts = ar.upload(p.consts, (size_t)p.S * MPCX_NCONST);
}

// a workspace cut into regions, each rounded up to 256 bytes
struct Carver {
    char *base, *p;
    explicit Carver(void *b) : base((char *)b), p((char *)b) {}
    template <typename T> T *take(size_t n)
    {
        T *r = (T *)p;
        p += (n * sizeof(T) + 255) & ~(size_t)255;
        return r;
    }
    size_t bytes() const { return (size_t)(p - base); }
};

// A set of V trajectories (rows of K nodes) flown again from their first node under a thrust table, as the refine loops and the Monte
// Carlo fly them: what the flight reads -- node counts, first nodes, tf, end_tau = 1, constants, the table Ut [V][3][K] -- and what it
// writes: Yp [V][7][K], status and step count.  A plain set of pointers: kernels take it by value.
struct FlightSet {
    int32_t *Ks, *pst, *nsteps;
    double *y0, *Ut, *tf, *end_tau, *consts, *Yp;
    // all nine regions, for a caller that owns them all
    void carve(Carver &c, size_t V, size_t K)
    {
        Ks = c.take<int32_t>(V); pst = c.take<int32_t>(V); nsteps = c.take<int32_t>(V);
        y0 = c.take<double>(V * 7); Ut = c.take<double>(V * 3 * K); tf = c.take<double>(V); end_tau = c.take<double>(V);
        consts = c.take<double>(V * MPCX_NCONST); Yp = c.take<double>(V * 7 * K);
    }
    // the flight: every trajectory over its whole table under the model `flags` with the step limit max_step
    int fly(mpcx_ctx *ctx, int V, int K, int flags, double max_step, hipStream_t stream) const
    {
        return mpcx_propagate_batch_ragged_dev(ctx, V, K, Ks, y0, tf, consts, flags, MPCX_CTRL_SEQUENCE, Ut, K, Ks, end_tau, max_step, Yp, pst, nsteps,
                                               stream);
    }
};

// the regions every linearising call's workspace starts with: [stage S (K-1) records][tf S][discretiser status S]
struct LinWorkspace {
    double *stage, *tf;
    int32_t *dstat;
    void carve(Carver &c, int S, int K)
    {
        stage = c.take<double>((size_t)S * (K - 1) * MPCX_STAGE_DOUBLES);
        tf = c.take<double>((size_t)S);
        dstat = c.take<int32_t>((size_t)S);
    }
};

// a workspace that is the linearisation's regions and nothing else, with its size (mpcx_covariance_thrust_batch_dev's)
struct LinOnlyWorkspace : LinWorkspace {
    size_t bytes;
    LinOnlyWorkspace(void *base, int S, int K)
    {
        Carver c(base);
        carve(c, S, K);
        bytes = c.bytes();
    }
};

// the argument tests of the covariance chains (`name`: covariance, covariance_thrust or covariance_drag)
inline int cov_check(mpcx_ctx *ctx, const char *name, int S, int K, int flags, double max_step)
{
    if (S < 1 || K < 2) return enc_fail(ctx, name, "need S>=1, K>=2");
    if (!(max_step > 0.0)) return enc_fail(ctx, name, "max_step must be > 0");
    if (flags & ~(MPCX_FLAG_DRAG | MPCX_FLAG_J2 | MPCX_FLAG_ATMO)) return enc_fail(ctx, name, "flags are MPCX_FLAG_DRAG | MPCX_FLAG_J2 | MPCX_FLAG_ATMO");
    return ctx_check_atmosphere(ctx, flags, name);
}

// The linearisation about (p.Y, p.U) under p.flags, p.max_step: tf [S], the span in each satellite's own time unit (1 where that is
// not positive and finite: the discretiser's step-size control never sees a value it was not written for, and the kernels that read
// the records make the same test and give that satellite MPCX_ST_BADK), then the stage records and the discretiser's status.
// Reads S, K, Ks, Y, U, units, span, consts, flags, max_step of p.  drag_column: the records carry the drag column G_k in their
// Sigma slot (MPCX_FLAG_DRAG_COLUMN; p.flags must contain MPCX_FLAG_DRAG) -- asked for here, not in p.flags, whose validation
// stays what it is.  (collision.hip)
int enc_linearise(mpcx_ctx *ctx, const EncProblem &p, const LinWorkspace &ws, hipStream_t stream, bool drag_column = false);

// mpcx_collision_window_sensitivity* as its entry points take it, and as mpcx_avoidance_window* (avoidance_window.hip) runs it
// first: the problem (its `target` is not read), the window call's own arguments, who moves, the outputs
struct CwsCall : EncProblem {
    const double *half;
    int panels, who;
    double *out, *sens, *state_grad;
    int32_t *status;
};

// workspace of the sensitivity: [the linearisation's][node sources n 2 K 6]
struct CwsWorkspace : LinWorkspace {
    double *src;
    void carve_cws(Carver &c, int n, int S, int K)
    {
        carve(c, S, K);
        src = c.take<double>((size_t)n * 2 * K * 6);
    }
};

// The argument tests of both calls (`name` in the messages) and the sensitivity kernel on linearised stage records.  (collision_window.hip)
int cws_check(mpcx_ctx *ctx, const CwsCall &c, const char *name, bool outputs_given, const char *outputs);
int cws_enqueue(mpcx_ctx *ctx, const CwsCall &c, const CwsWorkspace &ws, hipStream_t stream);

// mpcx_avoidance_window* as its entry points take it, and as mpcx_avoidance_window_refine* (avoidance_window_refine.hip) runs it
// as its pass 0
struct AwCall : CwsCall {
    double tol;
    int max_eval;
    double *du;
};
// the arguments of an entry point of either, under their names in include/mpcx.h, as an AwCall
#define MPCX_AW_CALL \
    AwCall{{MPCX_ENC_PROBLEM(radius, cat_radius, target_p), half_window, panels, who, out, sens, nullptr, status}, tol, max_eval, du}

// The argument tests of mpcx_avoidance_window* and the call itself on a workspace of mpcx_avoidance_window_workspace_bytes(n, S, K,
// panels) bytes.  (avoidance_window.hip)
int aw_check(mpcx_ctx *ctx, const AwCall &c, const char *name);
int aw_enqueue(mpcx_ctx *ctx, const AwCall &c, void *workspace, hipStream_t stream);

// mpcx_covariance_batch's chain over stage records that are there already: P [S][K][6][6] and status [S] from P0 [S][6][6], q [S]
// or NULL.  (collision.hip)
int cov_enqueue(mpcx_ctx *ctx, int S, int K, const int32_t *Ks, const double *stage, const int32_t *dstat, const double *units,
                const double *span, const double *P0, const double *q, double *P, int32_t *status, hipStream_t stream);

}  // namespace mpcx
