// encounter_host.hpp -- the host side that mpcx_avoidance*, mpcx_avoidance_joint*, mpcx_avoidance_refine*,
// mpcx_collision_window_sensitivity*, mpcx_avoidance_window* and mpcx_avoidance_window_refine* share, and the linearisation step they share with
// mpcx_covariance_batch*: the description of the problem, its argument tests and uploads, the workspace carver, and the set of
// trajectories that mpcx_avoidance_refine*, mpcx_avoidance_window_refine* and mpcx_collision_probability_mc* fly again (FlightSet).
#pragma once
#include "collision_device.hpp"                                     // CpSide
#include "mpcx_host.hpp"

namespace mpcx {

// a listed-pairs problem as every avoidance entry point takes it: the list, the plan that was screened, the model of its linearisation,
// the covariances and the catalogue (both optional), the target
struct EncProblem {
    int n;
    const double *pairs;
    int S, K;
    const int32_t *Ks;
    const double *Y, *U, *units, *span, *consts;
    int flags;
    double max_step;
    const double *P;
    int D, cat_K;
    const int32_t *cat_Ks;
    const double *cat_Y, *cat_units, *cat_span, *cat_P;
    double mu, target;
};

inline int enc_fail(mpcx_ctx *ctx, const char *name, const char *what)
{
    char msg[256];
    snprintf(msg, sizeof msg, "%s: %s", name, what);
    return ctx_fail(ctx, MPCX_E_BADARG, msg);
}

// The argument tests of the call `name` that every avoidance entry point makes.  outputs_given / outputs: whether the call's own
// required output arrays are all there, and their names as the message lists them behind the inputs.
inline int enc_check(mpcx_ctx *ctx, const EncProblem &p, const char *name, bool outputs_given, const char *outputs)
{
    if (p.n < 1 || p.S < 1 || p.K < 2 || !(p.mu > 0.0)) return enc_fail(ctx, name, "need n>=1, S>=1, K>=2, mu>0");
    if (!(p.target > 0.0) || !(p.target < __builtin_inf())) return enc_fail(ctx, name, "target must be a positive finite number");
    if (!(p.max_step > 0.0)) return enc_fail(ctx, name, "max_step must be > 0");
    if (p.flags & ~(MPCX_FLAG_DRAG | MPCX_FLAG_J2 | MPCX_FLAG_ATMO))
        return enc_fail(ctx, name, "flags are MPCX_FLAG_DRAG | MPCX_FLAG_J2 | MPCX_FLAG_ATMO");
    if (!p.pairs || !p.Y || !p.U || !p.units || !p.span || !p.consts || !outputs_given) {
        char what[192];
        snprintf(what, sizeof what, "pairs, Y, U, units, span, consts, %s are required", outputs);
        return enc_fail(ctx, name, what);
    }
    if (p.cat_Y) {
        if (p.D < 1 || p.cat_K < 2) return enc_fail(ctx, name, "a catalogue needs D>=1, cat_K>=2");
        if (!p.cat_units || !p.cat_span) return enc_fail(ctx, name, "cat_units and cat_span are required with cat_Y");
        if ((p.P != nullptr) != (p.cat_P != nullptr))
            return enc_fail(ctx, name, "P and cat_P come together (a Mahalanobis target) or not at all (metres)");
    }
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
    const size_t S = (size_t)p.S, K = (size_t)p.K, D = (size_t)p.D, cK = (size_t)p.cat_K;
    p.pairs = ar.upload(p.pairs, (size_t)p.n * 4);
    p.Y = ar.upload(p.Y, S * 7 * K); p.U = ar.upload(p.U, S * 3 * K);
    p.units = ar.upload(p.units, S * 2); p.span = ar.upload(p.span, S * 2); p.consts = ar.upload(p.consts, S * MPCX_NCONST);
    p.Ks = p.Ks ? ar.upload(p.Ks, S) : nullptr;
    p.P = p.P ? ar.upload(p.P, S * K * 36) : nullptr;
    if (p.cat_Y) {
        p.cat_Y = ar.upload(p.cat_Y, D * 7 * cK); p.cat_units = ar.upload(p.cat_units, D * 2);
        p.cat_span = ar.upload(p.cat_span, D * 2);
        p.cat_P = p.cat_P ? ar.upload(p.cat_P, D * cK * 36) : nullptr;
        p.cat_Ks = p.cat_Ks ? ar.upload(p.cat_Ks, D) : nullptr;
    }
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

// the argument tests of both covariance chains (`name`: covariance or covariance_thrust)
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
// Reads S, K, Ks, Y, U, units, span, consts, flags, max_step of p.  (collision.hip)
int enc_linearise(mpcx_ctx *ctx, const EncProblem &p, const LinWorkspace &ws, hipStream_t stream);

// mpcx_collision_window_sensitivity* as its entry points take it, and as mpcx_avoidance_window* (avoidance_window.hip) runs it
// first: the problem (its `target` is not read), the window call's own arguments, who moves, the outputs
struct CwsCall : EncProblem {
    const double *radius, *cat_radius, *half;
    int panels, who;
    double *out, *sens, *state_grad;
    int32_t *status;
};

// The two sides of the list of a window call (CwsCall, or collision_window.hip's CwCall: the same names) as its kernels take them:
// the constellation, and the catalogue where there is one, else the constellation again.
template <typename Call> inline void enc_sides(const Call &c, CpSide &row, CpSide &col)
{
    row = CpSide{c.S, c.K, c.Ks, c.Y, c.units, c.span, c.P, c.radius};
    col = c.cat_Y ? CpSide{c.D, c.cat_K, c.cat_Ks, c.cat_Y, c.cat_units, c.cat_span, c.cat_P, c.cat_radius} : row;
}

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
// the call's host arrays replaced by copies on the device
void cws_upload(DeviceArena &ar, CwsCall &c);

// mpcx_avoidance_window* as its entry points take it, and as mpcx_avoidance_window_refine* (avoidance_window_refine.hip) runs it
// as its pass 0
struct AwCall : CwsCall {
    double tol;
    int max_eval;
    double *du;
};
// the arguments of an entry point of either, under their names in include/mpcx.h, as an AwCall
#define MPCX_AW_CALL                                                                                                                  \
    AwCall{{{n, pairs, S, K, Ks, Y, U, units, span, consts, flags, max_step, P, D, cat_K, cat_Ks, cat_Y, cat_units, cat_span, cat_P, \
             mu, target_p}, radius, cat_radius, half_window, panels, who, out, sens, nullptr, status}, tol, max_eval, du}

// The argument tests of mpcx_avoidance_window* and the call itself on a workspace of mpcx_avoidance_window_workspace_bytes(n, S, K,
// panels) bytes.  (avoidance_window.hip)
int aw_check(mpcx_ctx *ctx, const AwCall &c, const char *name);
int aw_enqueue(mpcx_ctx *ctx, const AwCall &c, void *workspace, hipStream_t stream);

// mpcx_covariance_batch's chain over stage records that are there already: P [S][K][6][6] and status [S] from P0 [S][6][6], q [S]
// or NULL.  (collision.hip)
int cov_enqueue(mpcx_ctx *ctx, int S, int K, const int32_t *Ks, const double *stage, const int32_t *dstat, const double *units,
                const double *span, const double *P0, const double *q, double *P, int32_t *status, hipStream_t stream);

}  // namespace mpcx
