"""Inputs of the discretiser comparisons where max_step does not clip the steps: the one list that
tests/golden/make_discretize_unclipped_golden.py (the reference's arrays for them), tests/test_discretize_unclipped_host.py (the
oracle against those arrays, and every condition below) and tests/test_discretize_unclipped_gpu.py (discretize_kernel against the
oracle) share, with the oracle's results for them, its step and attempt counts, and the tolerance each (case, mode) is held to.

Every other device test of the discretiser but one runs at ivp_max_step = 1e-2, where each step is max_step long, no attempt is
rejected and the controller's pow is never evaluated.  Here max_step is 1 (and inf, and 2): the intervals are a quarter of an
orbit to two and a half, the controller rejects attempts in some groups of a wave and not in others, a step holds none, one or
several uniform points and spans several columns of the thrust table.

Cases (case(name)):
  plain, plain+j2   the inputs of test_discretize_step_factor_gpu.rejecting_case: S = 7, K = 4, Ku = 13 -- 21 intervals in three
                    waves, the last with five live groups
  drag-fixed, drag-general
                    satellites 0, 1, 4 of drag_cases.batch() with S x 1e2 and 1.5 times their tf, K = 4, Ku = 13, drag + J2 under
                    the fixed density and under the general atmosphere; a ragged launch, Ks = (4, 3, 4) with NaN behind the
                    middle satellite's columns (it has its own three nodes) -- nine slots in two waves, the second with one group,
                    one slot a shadow.  drag-general-k4: the same with Ks = 4 throughout (the reference layout is not ragged).
                    The thrust tables are those of a draw for the whole batch, rng(7).normal((5, 3, 13)) / 2, of which these
                    three satellites take theirs: of tables drawn for the three alone only one interval rejects an attempt
                    under the fixed density, and the conditions below ask for two.
  one               S = 1, K = 2, Ku = 13, tf = 2.5: one live group in the only wave, one interval of the whole horizon
Modes (MODES): rk45, rk23, uniN = N uniform dense-output points under RK45, rk23+uni7.

The tolerance is the project's own for long intervals, RTOL_LONG = 1e-8 of tests/test_discretize_gpu.py (there for cond(Phi) of
1e3 .. 2e4), scaled with the oracle's worst cond(A_k) of the (case, mode): 1e-8 max(1, cond / 2e4), relative to each array's
magnitude per satellite.  tolerance() asserts before it returns that this is at most 1e-3 of what the oracle's arrays move
by, satellite by satellite, when its steps are clipped at max_step = 1e-2 -- a kernel on another step sequence cannot pass; the host
test asserts that it is at least ten times the difference between the oracle and the reference itself.  Both are measured on
the references, never on what is compared with them.  Everything is deterministic (seeded) and computed once per process."""
import functools
import hashlib

import numpy as np

import drag_cases as D
import oracle_lib as O
from test_discretize_step_factor_gpu import CST, KEYS, RTOL_LONG, _inputs, relerr

DRAG, J2, RK23 = O.FLAG_DRAG, O.FLAG_J2, O.FLAG_RK23
MAX_STEP, CLIPPED_STEP = 1.0, 1e-2
COND_LONG = 2e4                     # the condition number RTOL_LONG was set at
EDGE_REL = 1e-13
MODES = {"rk45": (0, 0), "rk23": (RK23, 0), "uni2": (0, 2), "uni5": (0, 5), "uni33": (0, 33), "rk23+uni7": (RK23, 7), "uni9": (0, 9)}
PLAIN_MODES = ("rk23", "uni2", "uni5", "uni33", "rk23+uni7")
DRAG_MODES = ("rk45", "rk23", "uni9")
ONE_MODES = ("rk23", "uni33")
DRAG_SATS, DRAG_KS, DRAG_K, DRAG_KU, DRAG_SEED, DRAG_TF = (0, 1, 4), (4, 3, 4), 4, 13, 7, 1.5
BAD_SAT, BAD_COMPONENT, BAD_NODE = 3, 0, 1          # the failing satellite of (A): x[3, 0, 1] = NaN


def base_mode(mode):
    """the adaptive mode whose step sequence `mode` takes (the uniform points are read off the same steps)"""
    return "rk23" if MODES[mode][0] & RK23 else "rk45"


def per_attempt(mode):
    """right-hand sides per attempted step (first-same-as-last: RK45 six, RK23 three)"""
    return 3 if MODES[mode][0] & RK23 else 6


def _make(name, x, u, tf, const, Ks, flags, model, modes):
    return dict(name=name, x=x, u=u, tf=np.asarray(tf, dtype=np.float64), const=const, Ks=np.asarray(Ks, dtype=np.int32), S=x.shape[0],
                K=x.shape[2], Ku=u.shape[2], flags=flags, model=model, modes=modes)


@functools.lru_cache(None)
def _drag_inputs():
    """per satellite of DRAG_SATS: (u (3,13), tf, const) -- the batch's satellite with S x 1e2 (drag_cases.ROLL_S_SCALE: S x 1e4 over a
    third of an orbit at 300 km is a re-entry)"""
    b = D.batch()
    table = np.random.default_rng(DRAG_SEED).normal(size=(len(b["tf"]), 3, DRAG_KU)) * 0.5
    out = []
    for s in DRAG_SATS:
        cst = b["const"][s].copy()
        cst[D.C_S] *= D.ROLL_S_SCALE / D.S_SCALE
        out.append((table[s], DRAG_TF * float(b["tf"][s]), cst, b["y0"][s]))
    return out


def _drag_case(name, model, Ks):
    """x: the nodes of the drag + J2 rollout of a tenth of the table (drag_cases._rollout), Ks[i] of them for satellite i"""
    parts = _drag_inputs()
    x = np.full((len(parts), 7, DRAG_K), np.nan)
    for i, ((u, tf, cst, y0), k) in enumerate(zip(parts, Ks)):
        x[i, :, :k] = D._rollout(y0, tf, cst, 0.1 * u, int(k))
    return _make(name, x, np.stack([p[0] for p in parts]), [p[1] for p in parts], np.stack([p[2] for p in parts]), Ks, DRAG | J2, model, DRAG_MODES)


@functools.lru_cache(None)
def case(name):
    if name in ("plain", "plain+j2"):
        x, u, tf = _inputs(2024, 7, 4, 13, (0.8, 2.5), 0.5)
        return _make(name, x, u, tf, np.tile(CST, (7, 1)), [4] * 7, J2 if name == "plain+j2" else 0, None, PLAIN_MODES)
    if name in ("drag-fixed", "drag-general"):
        return _drag_case(name, name[5:], DRAG_KS)
    if name == "drag-general-k4":
        return _drag_case(name, "general", (DRAG_K,) * 3)
    if name == "one":
        x, u, tf = _inputs(2024, 1, 2, 13, (2.5, 2.5), 0.5)
        assert tf[0] == 2.5
        return _make(name, x, u, tf, np.tile(CST, (1, 1)), [2], 0, None, ONE_MODES)
    raise KeyError(name)


PLAIN, DRAGS, ONE = ("plain", "plain+j2"), ("drag-fixed", "drag-general"), "one"
# every (case, mode) the fixture holds the reference's arrays for and the device is compared on
ANCHORED = [(n, m) for n in PLAIN for m in PLAIN_MODES] + [(n, m) for n in DRAGS for m in DRAG_MODES] + [(ONE, m) for m in ONE_MODES]


def atmosphere(c):
    return D.models()[c["model"]] if c["model"] else None


def sat_inputs(c, s, x=None):
    """(x (7,Ks), u (3,Ku), tf, const) of satellite s: its own columns, without the padding"""
    k = int(c["Ks"][s])
    return (c["x"] if x is None else x)[s][:, :k], c["u"][s], float(c["tf"][s]), c["const"][s]


def input_hash(name):
    """sha256 of the case's inputs as the launch gets them: what the fixture records of the inputs it was computed from"""
    c = case(name)
    h = hashlib.sha256()
    for k in ("x", "u", "tf", "const", "Ks"):
        h.update(np.ascontiguousarray(c[k]).tobytes())
    return h.hexdigest()


def moved_x(c):
    """x (1 + 1e-13 d), d standard normal: the knife-edge probe"""
    return c["x"] * (1.0 + EDGE_REL * np.random.default_rng(1).standard_normal(c["x"].shape))


def bad_x(c):
    x = c["x"].copy()
    x[BAD_SAT, BAD_COMPONENT, BAD_NODE] = np.nan
    return x


def run_oracle(c, mode, max_step=MAX_STEP, x=None, flags=None, model="own", sats=None):
    """the oracle's discretize of every satellite (or of `sats`) -> list of its dicts; adaptive modes with their node dump"""
    fl, uni = MODES[mode]
    atm = atmosphere(c) if model == "own" else (D.models()[model] if model else None)
    outs = []
    for s in (range(c["S"]) if sats is None else sats):
        xs, u, tf, cst = sat_inputs(c, s, x)
        o = O.discretize(xs, u, tf, cst, (c["flags"] if flags is None else flags) | fl, max_step=max_step, dump_nodes=(uni == 0), uniform_steps=uni,
                         atmosphere=atm, node_rows=1024)
        assert uni or o["status"] or len(o["node_t"]) == o["node_counts"].sum()
        outs.append(o)
    return outs


@functools.lru_cache(None)
def oracle(name, mode, max_step=MAX_STEP):
    """the oracle's results of a (case, mode): computed once, left unchanged"""
    return tuple(run_oracle(case(name), mode, max_step))


def intervals(outs, key):
    return np.concatenate([np.asarray(o[key]) for o in outs])


def counts(name, mode):
    """-> (accepted steps, rejected attempts) per interval, satellite after satellite.  A uniform mode takes the steps of its
    adaptive mode (its own node_counts are the uniform points); its evaluations must be that mode's."""
    own, base = oracle(name, mode), oracle(name, base_mode(mode))
    nfev = intervals(own, "node_nfev")
    assert np.array_equal(nfev, intervals(base, "node_nfev")), (name, mode)
    accepted = intervals(base, "node_counts") - 1
    assert ((nfev - 2) % per_attempt(mode) == 0).all()
    return accepted, (nfev - 2) // per_attempt(mode) - accepted


def launch_slots(c, per_interval):
    """per-interval figures -> per slot of the launch, S x (K - 1) of them: a slot past a satellite's last interval shadows it"""
    out, at = [], 0
    for k in c["Ks"]:
        mine = per_interval[at:at + k - 1]
        out.extend(mine[min(j, k - 2)] for j in range(c["K"] - 1))
        at += k - 1
    return np.array(out)


def _linspace01(K, j):
    return 1.0 if j == K - 1 else j * (1.0 / (K - 1)) + 0.0


def steps(name, mode):
    """the accepted steps of the mode's adaptive run: [(tau_k, tau_kp1, node times)] per interval"""
    c, out = case(name), []
    for s, o in enumerate(oracle(name, base_mode(mode))):
        k, ends = int(c["Ks"][s]), np.concatenate([[0], np.cumsum(o["node_counts"])])
        out.extend((_linspace01(k, j), _linspace01(k, j + 1), o["node_t"][ends[j]:ends[j + 1]]) for j in range(k - 1))
    return out


def points_per_step(name, mode):
    """uniform modes: how many of the interval's uniform points (after its start) each accepted step holds, per interval --
    t_old < te <= t, the points as the oracle and the kernel form them"""
    n = MODES[mode][1]
    out = []
    for t0, t1, nodes in steps(name, mode):
        ustep = (t1 - t0) / (n - 1)
        te = np.array([t1 if j == n - 1 else j * ustep + t0 for j in range(1, n)])
        out.append(np.array([((te > a) & (te <= b)).sum() for a, b in zip(nodes[:-1], nodes[1:])]))
        assert out[-1].sum() == n - 1
    return out


def table_intervals_per_step(name, mode):
    """how many intervals of the thrust table each accepted step reaches into (two: it crosses a column)"""
    m = case(name)["Ku"] - 1
    return np.concatenate([np.ceil(t[1:] * m - 1e-9) - np.floor(t[:-1] * m + 1e-9) for _, _, t in steps(name, mode)]).astype(int)


def largest_step(name, mode):
    return max(float(np.diff(t).max()) for _, _, t in steps(name, mode))


def worst_cond(name, mode):
    return max(float(np.linalg.cond(a)) for o in oracle(name, mode) for a in o["A"])


def distance(a, b):
    """two results of one satellite: the largest relative difference over the five arrays, each against its own magnitude"""
    return max(relerr(a[k], b[k]) for k in KEYS)


@functools.lru_cache(None)
def clipped_gap(name, mode):
    """per satellite: how far the oracle at max_step = 1e-2 is from the oracle at max_step = 1"""
    return tuple(distance(a, b) for a, b in zip(oracle(name, mode), oracle(name, mode, CLIPPED_STEP)))


@functools.lru_cache(None)
def tolerance(name, mode):
    """1e-8 max(1, cond / 2e4), after the guard that keeps it meaningful: 1e3 times below every satellite's clipped_gap"""
    tol = RTOL_LONG * max(1.0, worst_cond(name, mode) / COND_LONG)
    gap = clipped_gap(name, mode)
    assert tol <= 1e-3 * min(gap), (name, mode, tol, gap)
    return tol


def errors(got, ref):
    """got, ref: per satellite the five arrays -> {array: worst relative error over the satellites}"""
    worst = dict.fromkeys(KEYS, 0.0)
    for s, (g, o) in enumerate(zip(got, ref)):
        for k in KEYS:
            assert g[k].shape == o[k].shape, (s, k, g[k].shape, o[k].shape)
            worst[k] = max(worst[k], relerr(g[k], o[k]))
    return worst


def drag_shares(name, mode):
    """(B) per satellite: relerr of A against the run without DRAG, and (general) against the fixed density"""
    c, own = case(name), oracle(name, mode)
    none = run_oracle(c, mode, flags=c["flags"] & ~DRAG, model=None)
    fixed = run_oracle(c, mode, model=None) if atmosphere(c) is not None else None
    return ([relerr(a["A"], b["A"]) for a, b in zip(own, none)],
            [relerr(a["A"], b["A"]) for a, b in zip(own, fixed)] if fixed else None)


@functools.lru_cache(None)
def check_conditions(name, mode):
    """what the (case, mode) is there for, asserted on the oracle alone -> the record of profiles/discretize_unclipped.txt.
    Where every interval rejects (RK23 on the plain and on the drag cases: 1 to 18 attempts each) a wave cannot hold a clean
    interval beside a rejecting one; the rejection counts within a wave must differ instead.  `one` has one interval."""
    c, outs = case(name), oracle(name, mode)
    assert all(o["status"] == 0 for o in outs), (name, mode, [o["status"] for o in outs])
    accepted, rejected = counts(name, mode)
    rec = dict(accepted=accepted.tolist(), rejected=rejected.tolist())
    if name == ONE:
        assert rejected[0] >= 1, rejected
    else:
        assert (rejected > 0).sum() >= 2, (name, mode, rejected)
        slots = launch_slots(c, rejected)
        waves = [slots[i:i + 8] for i in range(0, len(slots), 8)]
        if (rejected > 0).all():
            assert MODES[mode][0] & RK23 and any(len(set(w.tolist())) > 1 for w in waves), (name, mode, rejected)
        else:
            assert any((w > 0).any() and (w == 0).any() for w in waves), (name, mode, rejected)
    uni = MODES[mode][1]
    if uni:
        pts = points_per_step(name, mode)
        rec["points"] = (min(int(p.min()) for p in pts), max(int(p.max()) for p in pts))
        if uni == 2:
            assert all(p[-1] == 1 and p.sum() == 1 for p in pts)             # the only point after the start lies in the last step
        else:
            # among the uniform modes of the case: a step with three points or more, and an accepted step with none
            fullest = max(max(int(p.max()) for p in points_per_step(name, m)) for m in c["modes"] if MODES[m][1] > 2)
            assert fullest >= 3, (name, fullest)
            assert min(min(int(p.min()) for p in points_per_step(name, m)) for m in c["modes"] if MODES[m][1] > 2) == 0, name
    rec["table_intervals"] = int(table_intervals_per_step(name, mode).max())
    assert rec["table_intervals"] >= 2, (name, mode)
    rec["largest_step"] = largest_step(name, mode)
    moved = run_oracle(c, mode, x=moved_x(c))
    assert all(m["status"] == 0 for m in moved) and np.array_equal(intervals(moved, "node_nfev"), intervals(outs, "node_nfev")), (name, mode, "knife edge")
    if c["flags"] & DRAG:
        share, against_fixed = drag_shares(name, mode)
        assert min(share) >= 1e-7 and (against_fixed is None or min(against_fixed) >= 1e-7), (name, mode, share, against_fixed)
        rec["drag_share"], rec["against_fixed"] = share, against_fixed
    rec["cond"] = worst_cond(name, mode)
    return rec
