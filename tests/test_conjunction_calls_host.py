"""What conjunction.py hands to libmpcx.so, pinned call by call without a device, and what ConstellationMPC hands to conjunction.py.
The recorder of test_wrapper_calls_host.py stands in for the library: every scenario checks the entry point's name, the argument
count against _ffi._SIGS, every scalar with its type, every input array (dtype, contiguity, shape, contents; None where the C
signature takes NULL) and every output buffer (dtype, contiguity, shape, zeroed status words).  Every entry point that has a block
form is also called with devices=[0, 0]: blocks of 2 and 1 rows, each with its rows of the batched inputs and the whole of the
others, writing into the arrays the result object returns.  The messages of the checks the wrappers share are pinned as full
strings.  Nothing is solved."""
import numpy as np
import pytest

from mpconstellation_amd import _ffi, conjunction as cj
from mpconstellation_amd.constants import MU_EARTH
from test_wrapper_calls_host import I32, Out, Recorder, check_array, check_call, f64, i32, rec      # noqa: F401 (rec: the fixture)

S, N, D, NC, M = 3, 5, 2, 4, 6
T0, T1 = 10.0, 60.0
BLOCKS = [(0, 2), (2, 1)]                                                # what devices=[0, 0] makes of three rows


def ramp(*shape, start=0.0):
    return start + 0.01 * np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape)


Y, U, UNITS, SPAN, CONSTS = ramp(S, 7, N, start=1.0), ramp(S, 3, N, start=2.0), ramp(S, 2, start=3.0), ramp(S, 2, start=4.0), ramp(S, 8, start=5.0)
P, P0 = ramp(S, N, 6, 6, start=6.0), ramp(6, 6, start=7.0)
CY, CUNITS, CSPAN, CP = ramp(D, 7, NC, start=8.0), ramp(D, 2, start=9.0), ramp(D, 2, start=10.0), ramp(D, NC, 6, 6, start=11.0)
EPH, CEPH = ramp(S, 6, M, start=12.0), ramp(D, 6, M, start=13.0)
NS, CNS = [5, 4, 3], [4, 3]
RADIUS, CRADIUS = [1.0, 2.0, 3.0], [4.0, 5.0]
PAIRS = f64([[0, 1, 100.0, 20.0], [2, 0, 200.0, 30.0], [1, 0, 300.0, 40.0]])      # (j < D, so the list serves a catalogue as well)
HALF, Q = [10.0, 20.0, 30.0], [0.1, 0.2, 0.3]
ATMO = f64([1.0, 2.0, 3.0, 4.0])
TRAJ = dict(Y=Y, units=UNITS, span=SPAN, M=M)
CAT_TRAJ = dict(cat_Y=CY, cat_units=CUNITS, cat_span=CSPAN, cat_ns=CNS)
CAT_RADII = (CY, CUNITS, CSPAN, CP, CRADIUS, CNS)                          # the catalogue of the probabilities and the window calls
CAT_PLAIN = (CY, CUNITS, CSPAN, CP, CNS)                                   # ... of avoidance and the joint calls


def traj(Y, units, span, ns=None, *more):
    """one side as the library takes it: count, row length, node counts, trajectories [, covariances][, radii]"""
    return [Y.shape[0], Y.shape[2], None if ns is None else i32(ns), Y, units, span, *more]


def absent(n):
    return [0, 0] + [None] * n


def model(full):
    """the model keywords of a call, and the flags and max_step the library gets for them"""
    if full:
        return dict(include_drag=True, include_J2=True, atmosphere=ATMO, max_step=2e-3), _ffi.FLAG_DRAG | _ffi.FLAG_J2 | _ffi.FLAG_ATMO, 2e-3
    return {}, 0, cj.DEFAULT_MAX_STEP


class Case:
    """one call of a wrapper: `call(**where)` makes it, `want(ctx, blk)` is what the library must get for the block `blk` of the
    batched rows, `outs` lists (argument index, result -> array, axis): where the result object must show what the block wrote --
    axis 0 / 1: the block's rows / columns of the array, "whole": the very array, "first": the first block's own array"""

    def __init__(self, name, total, call, want, outs, marks=(), atmosphere=False):
        self.name, self.total, self.call, self.want, self.outs, self.marks, self.atmosphere = name, total, call, want, outs, marks, atmosphere


def list_rows(full, single):
    """a list of 3 rows, 2 with a catalogue; under two blocks always 3, so that the blocks are unequal"""
    return PAIRS[:2] if full and single else PAIRS


def list_case(kind, from_traj, full, single):
    rows = list_rows(full, single)
    fn = {"pairs": cj.screen_pairs, "events": cj.screen_events, "track": cj.screen_track}[kind]
    kw, scalars = {"pairs": ({}, []), "events": (dict(threshold=50.0, max_events=2), [50.0, 2]) if full else ({}, [0.0, 16]),
                   "track": (dict(max_shift=7.0), [7.0]) if full else ({}, [0.0])}[kind]
    E = 2 if full else 16
    if from_traj:
        sides = dict(TRAJ, ns=NS, **CAT_TRAJ) if full else dict(TRAJ)
    else:
        sides = dict(eph=EPH, cat_eph=CEPH) if full else dict(eph=EPH)

    def want(ctx, blk):
        c = blk.stop - blk.start
        outs = {"pairs": [Out(c, 4), Out(c, dtype=I32, zero=True)],
                "events": [Out(c, E, 4), Out(c, E, 2, dtype=I32), Out(c, dtype=I32, zero=True), Out(c, dtype=I32, zero=True)],
                "track": [Out(c, 4), Out(c, 2, dtype=I32), Out(c, dtype=I32, zero=True)]}[kind]
        if from_traj:
            return [ctx, c, rows[blk]] + traj(Y, UNITS, SPAN, NS if full else None) + (traj(CY, CUNITS, CSPAN, CNS) if full else absent(4)) \
                + [M, T0, T1] + scalars + outs + [Out(S, dtype=I32, zero=True), Out(D, dtype=I32, zero=True) if full else None]
        return [ctx, c, rows[blk], S, D if full else 0, M, EPH, CEPH if full else None, T0, T1] + scalars + outs
    k = 2 if from_traj else 0                                           # (the two ephemeris statuses come last)
    if kind == "events":
        outs, marks = [(-2 - k, lambda r: r.count, 0), (-1 - k, lambda r: r.status, 0)], []
        statuses = [(-2, lambda r: r.eph_status, "first"), (-1, lambda r: r.cat_status, "first")]
    else:
        m = 3 if kind == "track" else 2                                 # out [, info], status
        outs = [(i - m - k, (lambda r, i=i: r[i]), 0) for i in range(m)]
        marks = [o[0] for o in outs[:-1]]
        statuses = [(-2, lambda r: r[m], "first"), (-1, lambda r: r[m + 1], "first")]
    name = "mpcx_conjunction_" + kind + ("_traj" if from_traj else "")
    return Case(name, len(rows), lambda **where: fn(rows, T0, T1, **kw, **sides, **where), want, outs + (statuses if from_traj else []), marks=marks)


def covariance_case(thrust, full, single):
    mkw, flags, max_step = model(full)
    mv = [0.5, 0.6, 0.7]
    execution = ramp(S, 5) if full else ramp(5)
    kw = dict(ns=NS, q=Q) if full else {}

    def call(**where):
        if thrust:
            return cj.covariance_thrust(Y, UNITS, SPAN, CONSTS, P0, U, execution, mass_var0=mv if full else None, return_mass=full,
                                        return_status=True, **kw, **mkw, **where)
        return cj.covariance(Y, UNITS, SPAN, CONSTS, P0, U=U if full else None, return_status=True, **kw, **mkw, **where)

    def want(ctx, blk):
        c = blk.stop - blk.start
        w = [ctx, c, N, i32(NS)[blk] if full else None, Y[blk], U[blk] if thrust or full else None, UNITS[blk], SPAN[blk], CONSTS[blk], flags,
             max_step, f64(np.broadcast_to(P0, (c, 6, 6))), f64(Q)[blk] if full else None]
        if thrust:
            w += [f64(np.broadcast_to(execution, (S, 5)))[blk], f64(mv)[blk] if full else None]
        return w + [Out(c, N, 6, 6)] + ([Out(c, N, 7) if full else None] if thrust else []) + [Out(c, dtype=I32, zero=True)]
    outs = [(-3, lambda r: r[0], 0), (-2, lambda r: r[1] if full else None, 0), (-1, lambda r: r[-1], 0)] if thrust else \
           [(-2, lambda r: r[0], 0), (-1, lambda r: r[1], 0)]
    return Case("mpcx_covariance_thrust_batch" if thrust else "mpcx_covariance_batch", S, call, want, outs,
                marks=([-3, -2] if full else [-3]) if thrust else [-2], atmosphere=full)


def probability_case(window, full, single):
    rows = list_rows(full, single)
    radius, mu = (RADIUS, 4.0e14) if full else (5.0, float(MU_EARTH))
    half, panels = (HALF[:len(rows)], 3) if full else (10.0, 4)
    kw = dict(ns=NS, cat=CAT_RADII, mu=mu) if full else {}

    def call(**where):
        if window:
            return cj.collision_probability_window(rows, radius, Y, UNITS, SPAN, P, half, **({"panels": 3} if full else {}), **kw, **where)
        return cj.collision_probability(rows, radius, Y, UNITS, SPAN, P, **kw, **where)

    def want(ctx, blk):
        c = blk.stop - blk.start
        w = [ctx, c, rows[blk]] + traj(Y, UNITS, SPAN, NS if full else None, P, f64(RADIUS) if full else np.full(S, 5.0)) \
            + (traj(CY, CUNITS, CSPAN, CNS, CP, f64(CRADIUS)) if full else absent(6)) + [mu]
        if window:
            w += [f64(half)[blk] if full else np.full(c, 10.0), panels]
        return w + [Out(c, _ffi.NPW if window else _ffi.NPC), Out(c, dtype=I32, zero=True)]
    outs = [(-2, (lambda r: r.p) if window else (lambda r: r.pc), 0), (-1, lambda r: r.status, 0)]
    return Case("mpcx_collision_probability_window" if window else "mpcx_collision_probability", len(rows), call, want, outs, marks=[-2])


def plan_side(full, flags, max_step, covariances):
    """the plan as the avoidance calls hand it over, up to the covariances"""
    return [S, N, i32(NS) if full else None, Y, U, UNITS, SPAN, CONSTS, flags, max_step, covariances]


def avoidance_case(full, single):
    rows = list_rows(full, single)
    mkw, flags, max_step = model(full)
    kw = dict(ns=NS, P=P, cat=CAT_PLAIN, mu=4.0e14, return_sensitivities=True) if full else dict(who="both")
    NSL = 1 if full else 2

    def want(ctx, blk):
        c = blk.stop - blk.start
        return [ctx, c, rows[blk]] + plan_side(full, flags, max_step, P if full else None) + (traj(CY, CUNITS, CSPAN, CNS, CP) if full else absent(5)) \
            + [4.0e14 if full else float(MU_EARTH), 500.0, 0 if full else 2, Out(c, _ffi.NAV), Out(c, NSL, 3, N), Out(c, NSL, 3, 3, N) if full else None,
               Out(c, dtype=I32, zero=True)]
    outs = [(-4, lambda r: r.out, 0), (-3, lambda r: r.du, 0), (-2, lambda r: r.sens, 0), (-1, lambda r: r.status, 0)]
    return Case("mpcx_avoidance", len(rows), lambda **where: cj.avoidance(rows, 500.0, Y, U, UNITS, SPAN, CONSTS, **kw, **mkw, **where), want, outs,
                marks=[-4, -3, -2] if full else [-4, -3], atmosphere=full)


def window_case(kind, full, single):
    """collision_window_sensitivity ("sens"), avoidance_window ("avoid") and avoidance_window_refine ("refine")"""
    rows = list_rows(full, single)
    mkw, flags, max_step = model(full)
    half, panels, mu = (HALF[:len(rows)], 3, 4.0e14) if full else (10.0, 4, float(MU_EARTH))
    kw = dict(ns=NS, cat=CAT_RADII, mu=mu, panels=3) if full else dict(who="j")
    NSL, rounds = (1, 1) if full else (2, 2)
    target = [] if kind == "sens" else [0.001, 1e-4, 9] if full else [0.001, _ffi.AW_DEFAULT_TOL, _ffi.AW_DEFAULT_MAX_EVAL]
    tkw = dict(tol=1e-4, max_eval=9) if full and kind != "sens" else {}

    def call(**where):
        if kind == "sens":
            return cj.collision_window_sensitivity(rows, RADIUS if full else 5.0, Y, U, UNITS, SPAN, CONSTS, P, half, return_state_gradient=full,
                                                   **kw, **mkw, **where)
        if kind == "avoid":
            return cj.avoidance_window(rows, 0.001, RADIUS if full else 5.0, Y, U, UNITS, SPAN, CONSTS, P, half, return_sensitivities=full,
                                       **kw, **tkw, **mkw, **where)
        more = dict(rounds=1, track=(M, T0, T1), max_shift=7.0, recov=True, q=0.5, prop_max_step=2e-4) if full else {}
        return cj.avoidance_window_refine(rows, 0.001, RADIUS if full else 5.0, Y, U, UNITS, SPAN, CONSTS, P, half, return_sensitivities=full,
                                          **more, **kw, **tkw, **mkw, **where)

    def want(ctx, blk):
        c = blk.stop - blk.start
        w = [ctx, c, rows[blk]] + plan_side(full, flags, max_step, P) + [f64(RADIUS) if full else np.full(S, 5.0)] \
            + (traj(CY, CUNITS, CSPAN, CNS, CP, f64(CRADIUS)) if full else absent(6)) \
            + [mu, f64(half)[blk] if full else np.full(c, 10.0), panels, 0 if full else 1] + target
        status = Out(c, dtype=I32, zero=True)
        if kind == "sens":
            return w + [Out(c, _ffi.NPW), Out(c, NSL, 3, N), Out(c, 64 * 3 + 1, 6) if full else None, status]
        w += [] if kind == "avoid" else ([2e-4, 1, M, T0, T1, 7.0, 1, np.full(S, 0.5)] if full else [1e-3, 2, 0, 0.0, 0.0, 0.0, 0, None])
        w += [Out(c, _ffi.NAW), Out(c, NSL, 3, N), Out(c, NSL, 3, N) if full else None, status]
        if kind == "refine":
            w += [np.full(c, -1, dtype=I32), Out(c, NSL, 7, N), Out(c, NSL, N, 6, 6) if full else None, Out(rounds + 2, c), Out(rounds + 2, c),
                  Out(rounds + 1, c)]
        return w
    name = {"sens": "mpcx_collision_window_sensitivity", "avoid": "mpcx_avoidance_window", "refine": "mpcx_avoidance_window_refine"}[kind]
    if kind == "sens":
        outs = [(-4, lambda r: r.p, 0), (-3, lambda r: r.sens, 0), (-2, lambda r: r.state_grad, 0), (-1, lambda r: r.status, 0)]
        marks = [-4, -3, -2] if full else [-4, -3]
    else:
        o = -6 if kind == "refine" else 0
        outs = [(o - 4, lambda r: r.out, 0), (o - 3, lambda r: r.du, 0), (o - 2, lambda r: r.sens, 0), (o - 1, lambda r: r.status, 0)]
        marks = [o - 4, o - 3, o - 2] if full else [o - 4, o - 3]
        if kind == "refine":
            outs += [(-6, lambda r: r.rounds_done, 0), (-5, lambda r: r.Y_flown, 0), (-4, lambda r: r.P_flown, 0), (-3, lambda r: r.p_history, 1),
                     (-2, lambda r: r.t_history, 1), (-1, lambda r: r.p_predicted, 1)]
            marks += [-5, -3, -2, -1] + ([-4] if full else [])
    return Case(name, len(rows), call, want, outs, marks=marks, atmosphere=full)


def joint_tail(full, n):
    return [Out(S, 3, N, zero=True), Out(S, _ffi.NAJ, zero=True), Out(n, _ffi.NAR, zero=True), Out(n, 3, N, zero=True) if full else None,
            Out(S, 6, 3, N, zero=True) if full else None, Out(S, dtype=I32, zero=True), Out(n, dtype=I32, zero=True)]


JOINT_OUTS = [(-7, lambda r: r.du, "whole"), (-6, lambda r: r.sat_out, "whole"), (-5, lambda r: r.row_out, "whole"), (-4, lambda r: r.rows, "whole"),
              (-3, lambda r: r.tsens, "whole"), (-2, lambda r: r.status, "whole"), (-1, lambda r: r.row_status, "whole")]


def joint_head(rows, full, flags, max_step):
    """the list, the plan and the problem of the joint calls, up to max_iter"""
    return [len(rows), rows, i32([0] * len(rows)) if full else i32([1, 0, 1])] + plan_side(full, flags, max_step, P if full else None) \
        + (traj(CY, CUNITS, CSPAN, CNS, CP) if full else absent(5)) \
        + ([4.0e14, 500.0, f64([0.5, 0.6, 0.7]), 0, 1e-8, 7] if full else [float(MU_EARTH), 500.0, None, 1, _ffi.AJ_DEFAULT_TOL, _ffi.AJ_DEFAULT_MAX_ITER])


def joint_kw(full):
    if full:
        return dict(ns=NS, P=P, cat=CAT_PLAIN, mu=4.0e14, u_max=[0.5, 0.6, 0.7], hold_terminal=False, tol=1e-8, max_iter=7, return_rows=True,
                    return_terminal=True)
    return dict(who=np.array([1, 0, 1]))


def joint_case(full, single):
    rows = list_rows(full, single)
    mkw, flags, max_step = model(full)

    def want(ctx, blk):                                                 # the blocks are blocks of SATELLITES; every one gets the whole list
        return [ctx] + joint_head(rows, full, flags, max_step) + [blk.start, blk.stop - blk.start] + joint_tail(full, len(rows))
    return Case("mpcx_avoidance_joint", S, lambda **where: cj.avoidance_joint(rows, 500.0, Y, U, UNITS, SPAN, CONSTS, **joint_kw(full), **mkw, **where),
                want, JOINT_OUTS, atmosphere=full)


def refine_case(tracked, full, single):
    rows = list_rows(full, single)
    mkw, flags, max_step = model(full)
    n, rounds = len(rows), 1 if full else 3
    kw = dict(joint_kw(full), rounds=1, prop_max_step=2e-4, return_rhs=True) if full else joint_kw(full)
    if tracked:
        kw.update(track=True, **({"max_shift": 7.0} if full else {}))

    def want(ctx, blk):
        return [ctx] + joint_head(rows, full, flags, max_step) + [M, T0, T1, 2e-4 if full else 1e-3, rounds] + ([7.0 if full else 0.0] if tracked else []) \
            + joint_tail(full, n) + [Y, rows, Out(rounds + 2, n, zero=True), Out(rounds + 2, n, zero=True), Out(rounds + 2, S, zero=True),
                                     np.full(S, -1, dtype=I32), Out(n, zero=True) if full else None, Out(S, 6, zero=True) if full else None]
    outs = [(i - 8, get, ax) for i, get, ax in JOINT_OUTS] + \
           [(-8, lambda r: r.Y_flown, "whole"), (-7, lambda r: r.pairs_flown, "whole"), (-6, lambda r: r.d0_history, "whole"),
            (-5, lambda r: r.tca_history, "whole"), (-4, lambda r: r.terminal_history, "whole"), (-3, lambda r: r.rounds_done, "whole"),
            (-2, lambda r: r.rhs_rows, "whole"), (-1, lambda r: r.rhs_term, "whole")]
    return Case("mpcx_avoidance_refine_tracked" if tracked else "mpcx_avoidance_refine", S,
                lambda **where: cj.avoidance_refine(rows, 500.0, Y, U, UNITS, SPAN, CONSTS, M, T0, T1, **kw, **mkw, **where), want, outs, atmosphere=full)


BLOCK_CASES = {f"{kind}{'_traj' if t else ''}": (lambda full, single, kind=kind, t=t: list_case(kind, t, full, single))
               for kind in ("pairs", "events", "track") for t in (False, True)}
BLOCK_CASES.update({"covariance": lambda f, s: covariance_case(False, f, s), "covariance_thrust": lambda f, s: covariance_case(True, f, s),
                    "collision": lambda f, s: probability_case(False, f, s), "collision_window": lambda f, s: probability_case(True, f, s),
                    "avoidance": avoidance_case, "window_sensitivity": lambda f, s: window_case("sens", f, s),
                    "avoidance_window": lambda f, s: window_case("avoid", f, s), "avoidance_window_refine": lambda f, s: window_case("refine", f, s),
                    "avoidance_joint": joint_case})
ONE_DEVICE_CASES = dict(BLOCK_CASES, avoidance_refine=lambda f, s: refine_case(False, f, s), avoidance_refine_tracked=lambda f, s: refine_case(True, f, s))


def library_calls(rec, name):
    """the recorded calls without those that hand a context its atmosphere, which are checked here: one per context, before the call"""
    atmo = [c for c in rec.calls if c[0] == "mpcx_set_atmosphere"]
    rest = [c for c in rec.calls if c[0] != "mpcx_set_atmosphere"]
    assert all(c[0] == name for c in rest), [c[0] for c in rest]
    return rec.named(name), atmo


def check_atmosphere(rec, case, calls, atmo):
    assert len(atmo) == (len(calls) if case.atmosphere else 0)
    for c in calls:
        if case.atmosphere:
            given = [a for a in atmo if a[1][0] == c[1][0]]
            assert len(given) == 1 and rec.calls.index(given[0]) < rec.calls.index(c)
            check_array(given[0][1][1], ATMO, "atmosphere")


@pytest.mark.parametrize("full", [False, True], ids=["plain", "every option"])
@pytest.mark.parametrize("which", list(ONE_DEVICE_CASES))
def test_one_device(rec, which, full):
    case = ONE_DEVICE_CASES[which](full, True)
    res = case.call(device=1)
    calls, atmo = library_calls(rec, case.name)
    assert len(calls) == 1
    check_atmosphere(rec, case, calls, atmo)
    args = check_call(calls[0], case.name, case.want(("ctx", 1, 0), slice(0, case.total)))
    for i, get, _ in case.outs:
        a = get(res)
        if a is None:
            assert args[i] is None, i
        else:
            assert np.shares_memory(a, args[i]) and a.ctypes.data == args[i].ctypes.data and a.shape[0] == args[i].shape[0], i
    rec.calls.clear()
    case.call(devices=[2])                                              # a device list of one is that device
    assert [c[1][0] for c in rec.calls if c[0] == case.name] == [("ctx", 2, 0)]


@pytest.mark.parametrize("full", [False, True], ids=["plain", "every option"])
@pytest.mark.parametrize("which", list(BLOCK_CASES))
def test_two_blocks(rec, which, full):
    case = BLOCK_CASES[which](full, False)

    def library_writes(*a):
        for i in case.marks:
            a[i][...] = 1 + a[0][2]
    rec.on[case.name] = library_writes
    res = case.call(devices=[0, 0])
    calls, atmo = library_calls(rec, case.name)
    assert len(calls) == 2
    check_atmosphere(rec, case, calls, atmo)
    for slot, (first, count) in enumerate(BLOCKS):
        blk = slice(first, first + count)
        args = check_call(calls[slot], case.name, case.want(("ctx", 0, slot), blk))
        for i, get, axis in case.outs:
            a = get(res)
            if a is None:
                assert args[i] is None, i
            elif axis == "whole":
                assert args[i].ctypes.data == a.ctypes.data and args[i].shape[0] == a.shape[0], i
            elif axis == "first":
                assert args[i].shape == a.shape and (args[i].ctypes.data == a.ctypes.data) == (slot == 0), i
            elif axis == 0:
                assert np.shares_memory(args[i], a) and args[i].ctypes.data == a[blk].ctypes.data and len(a) == case.total, i
            if i in case.marks:
                back = a[blk] if axis == 0 else a[:, blk]
                assert back.size and (back == 1 + slot).all(), (i, back)


# ------------------------------------------------------------------------------------------------ the ephemeris and the screens
@pytest.mark.parametrize("ns", [None, NS])
def test_common_clock(rec, ns):
    eph, status = cj.common_clock(Y, UNITS, SPAN, M, T0, T1, ns=ns, device=1, return_status=True)
    args = check_call(rec.calls[0], "mpcx_ephemeris_batch",
                      [("ctx", 1, 0), S, N, None if ns is None else i32(ns), Y, UNITS, SPAN, M, T0, T1, Out(S, 6, M), Out(S, dtype=I32, zero=True)])
    assert args[4] is Y and eph is args[-2] and status is args[-1] and len(rec.calls) == 1
    assert cj.common_clock(Y, UNITS, SPAN, M, 10, 60) is rec.calls[1][1][-2] and type(rec.calls[1][1][8]) is float


class CountPointer:
    """the screens' n_pairs: a pointer to one int64"""

    def __eq__(self, other):
        return isinstance(other, _ffi._lp)


def screen_case(cross, from_traj, listing):
    fn = cj.screen_against if cross else cj.screen
    if from_traj:
        sides = dict(TRAJ, ns=NS, **(CAT_TRAJ if cross else {}))
    else:
        sides = dict(eph=EPH, **(dict(cat_eph=CEPH) if cross else {}))
    kw = dict(threshold=50.0, max_pairs=2) if listing else {}
    thr, max_pairs = (50.0, 2) if listing else (0.0, 0)

    def want(ctx, first, count):
        tail = [T0, T1, first, count, thr, max_pairs, Out(count), Out(count, dtype=I32), Out(count), Out(max_pairs, 4), CountPointer()]
        if from_traj:
            return [ctx] + traj(Y, UNITS, SPAN, NS) + (traj(CY, CUNITS, CSPAN, CNS) if cross else []) + [M] + tail \
                + [Out(S, dtype=I32, zero=True)] + ([Out(D, dtype=I32, zero=True)] if cross else [])
        return [ctx, S] + ([D] if cross else []) + [M, EPH] + ([CEPH] if cross else []) + tail
    name = "mpcx_conjunction_" + ("cross_screen" if cross else "screen") + ("_traj" if from_traj else "")
    return name, (lambda **where: fn(T0=T0, T1=T1, **sides, **kw, **where)), want


SCREENS = [(c, t) for c in (False, True) for t in (False, True)]


@pytest.mark.parametrize("listing", [False, True], ids=["no list", "list"])
@pytest.mark.parametrize("cross, from_traj", SCREENS)
def test_screen_one_device(rec, cross, from_traj, listing):
    name, call, want = screen_case(cross, from_traj, listing)
    k = (2 if cross else 1) if from_traj else 0
    found = f64([[1, 2, 30.0, 3.0], [0, 2, 20.0, 2.0]])

    def library_writes(*a):
        count = a[-1 - k]
        assert count[0] == 0                                            # (arrives zeroed)
        if listing:
            a[-2 - k][...] = found
            count[0] = 5                                                # two stored, five found
    rec.on[name] = library_writes
    res = call(device=1)
    args = check_call(rec.calls[0], name, want(("ctx", 1, 0), 0, S))
    assert len(rec.calls) == 1
    assert res.dmin is args[-5 - k] and res.partner is args[-4 - k] and res.tca is args[-3 - k]
    assert res.n_pairs_total == (5 if listing else 0) and type(res.n_pairs_total) is int
    check_array(res.pairs, found[::-1] if listing else np.zeros((0, 4)), "pairs")
    if from_traj:
        assert res.status is args[-k] and (res.cat_status is args[-1]) == cross and (res.cat_status is None) != cross
    else:
        assert res.status is None and res.cat_status is None


@pytest.mark.parametrize("cross, from_traj", SCREENS)
def test_screen_two_blocks_join_and_sort_their_lists(rec, cross, from_traj):
    name, call, want = screen_case(cross, from_traj, True)
    k = (2 if cross else 1) if from_traj else 0
    found = {0: (f64([[1, 2, 30.0, 3.0], [0, 2, 20.0, 2.0]]), 3), 1: (f64([[0, 1, 10.0, 1.0], [9, 9, 9.0, 9.0]]), 1)}

    def library_writes(*a):
        slot = a[0][2]
        a[-2 - k][...], a[-1 - k][0] = found[slot]
        for i in (-5 - k, -4 - k, -3 - k):
            a[i][...] = 1 + slot
    rec.on[name] = library_writes
    res = call(devices=[0, 0])
    calls = rec.named(name)
    assert len(calls) == 2 == len(rec.calls)
    for slot, (first, count) in enumerate(BLOCKS):
        args = check_call(calls[slot], name, want(("ctx", 0, slot), first, count))
        for a, whole in zip(args[-5 - k:-2 - k], (res.dmin, res.partner, res.tca)):
            assert a.ctypes.data == whole[first:].ctypes.data and (whole[first:first + count] == 1 + slot).all()
    # block 0 stores two of its three, block 1 its one (the fourth row of its buffer is not a pair); joined, sorted, cut at max_pairs
    check_array(res.pairs, f64([[0, 1, 10.0, 1.0], [0, 2, 20.0, 2.0]]), "pairs")
    assert res.n_pairs_total == 4 and res.dmin.shape == res.partner.shape == res.tca.shape == (S,) and res.partner.dtype == I32
    if from_traj:                                                       # the first block's ephemeris statuses
        first_block = calls[0][1]
        assert res.status is first_block[-k] and (res.cat_status is first_block[-1]) == cross


# ------------------------------------------------------------------------------------------------ every wrapper by name
GIVEN = dict(pairs=PAIRS, radius=5.0, Y=Y, U=U, units=UNITS, span=SPAN, consts=CONSTS, P=P, P0=P0, half_window=10.0, target=500.0, target_p=0.001,
             execution=np.zeros(5), M=M, T0=T0, T1=T1)
PUBLIC = {                                                               # every wrapper with the names of its positional arguments
    "screen_pairs": (cj.screen_pairs, "pairs T0 T1"), "screen_events": (cj.screen_events, "pairs T0 T1"), "screen_track": (cj.screen_track, "pairs T0 T1"),
    "collision_probability": (cj.collision_probability, "pairs radius Y units span P"),
    "collision_probability_window": (cj.collision_probability_window, "pairs radius Y units span P half_window"),
    "avoidance": (cj.avoidance, "pairs target Y U units span consts"),
    "collision_window_sensitivity": (cj.collision_window_sensitivity, "pairs radius Y U units span consts P half_window"),
    "avoidance_window": (cj.avoidance_window, "pairs target_p radius Y U units span consts P half_window"),
    "avoidance_window_refine": (cj.avoidance_window_refine, "pairs target_p radius Y U units span consts P half_window"),
    "avoidance_joint": (cj.avoidance_joint, "pairs target Y U units span consts"),
    "avoidance_refine": (cj.avoidance_refine, "pairs target Y U units span consts M T0 T1"),
    "covariance": (cj.covariance, "Y units span consts P0"),
    "covariance_thrust": (cj.covariance_thrust, "Y units span consts P0 U execution"),
}
LIST_CALLS = [f for f in PUBLIC if not f.startswith("covariance")]


def call(f, **kw):
    """wrapper f on the good arguments GIVEN (the list screens from trajectories), with those of kw in their place or added"""
    fn, names = PUBLIC[f]
    kw = {**(dict(Y=Y, units=UNITS, span=SPAN, M=M) if f.startswith("screen_") else {}), **kw}
    return fn(*[kw.pop(n) if n in kw else GIVEN[n] for n in names.split()], **kw)


WINDOW_CALLS = ("collision_probability_window", "collision_window_sensitivity", "avoidance_window", "avoidance_window_refine")
PLAN_CALLS = ("avoidance", "collision_window_sensitivity", "avoidance_window", "avoidance_window_refine", "avoidance_joint", "avoidance_refine")
RADII_CAT = ("collision_probability",) + WINDOW_CALLS

def test_events_come_back_from_both_blocks(rec):
    def library_writes(*a):
        slot = a[0][2]
        a[-4][:, 0, :], a[-3][:, 0, :], a[-2][...] = 1 + slot, (7 + slot, slot), 1
    rec.on["mpcx_conjunction_events"] = library_writes
    ev = cj.screen_events(PAIRS, T0, T1, max_events=2, eph=EPH, devices=[0, 0])
    check_array(ev.events, f64([[1] * 4, [1] * 4, [2] * 4]), "events")
    assert ev.row.tolist() == [0, 1, 2] and ev.interval.tolist() == [7, 7, 8] and ev.edge.tolist() == [False, False, True]
    assert ev.count.tolist() == [1, 1, 1] and not ev.truncated.any() and ev.max_events == 2 and ev.eph_status is None


def test_an_empty_list_makes_no_library_call(rec):
    none = np.zeros((0, 4))
    for where in (dict(device=1), dict(devices=[0, 0])):
        assert [a.shape for a in cj.screen_pairs(none, T0, T1, **TRAJ, **where)[:2]] == [(0, 4), (0,)] and cj.screen_pairs(none, T0, T1, **TRAJ)[2:] == (None, None)
        assert len(cj.screen_events(none, T0, T1, eph=EPH, **where).events) == 0
        assert [a.shape for a in cj.screen_track(none, T0, T1, eph=EPH, **where)] == [(0, 4), (0, 2), (0,)]
        assert cj.collision_probability(none, 5.0, Y, UNITS, SPAN, P, **where).pc.shape == (0,)
        assert cj.avoidance(none, 500.0, Y, U, UNITS, SPAN, CONSTS, **where).du.shape == (0, 2, 3, N)
        assert cj.collision_window_sensitivity(none, 5.0, Y, U, UNITS, SPAN, CONSTS, P, 10.0, **where).sens.shape == (0, 2, 3, N)
        assert cj.avoidance_window(none, 0.001, 5.0, Y, U, UNITS, SPAN, CONSTS, P, 10.0, **where).du.shape == (0, 2, 3, N)
        r = cj.avoidance_window_refine(none, 0.001, 5.0, Y, U, UNITS, SPAN, CONSTS, P, 10.0, **where)
        assert r.p_history.shape == (4, 0) and r.p_predicted.shape == (3, 0) and r.Y_flown.shape == (0, 2, 7, N) and r.P_flown is None
        j = cj.avoidance_joint(none, 500.0, Y, U, UNITS, SPAN, CONSTS, **where)
        assert j.du.shape == (S, 3, N) and not j.du.any() and j.coupled.shape == (0,)
    for f in PLAN_CALLS:                                                # (the checks do not depend on the list's length)
        with pytest.raises(ValueError, match="max_step: need > 0, got 0.0"):
            call(f, pairs=none, max_step=0.0)
    r = cj.avoidance_refine(none, 500.0, Y, U, UNITS, SPAN, CONSTS, M, T0, T1, rounds=1)
    assert r.d0_history.shape == (3, 0) and np.array_equal(r.Y_flown, Y) and r.Y_flown is not Y and (r.rounds_done == -1).all()
    assert rec.calls == []


def test_the_flags_carry_the_atmosphere_only_beside_the_drag(rec):
    cj.avoidance(PAIRS, 500.0, Y, U, UNITS, SPAN, CONSTS, include_J2=True, atmosphere=ATMO)
    cj.covariance(Y, UNITS, SPAN, CONSTS, P0, include_J2=True, atmosphere=ATMO)
    assert [c[0] for c in rec.calls] == ["mpcx_avoidance", "mpcx_covariance_batch"]
    assert rec.calls[0][1][11] == _ffi.FLAG_J2 == rec.calls[1][1][9]


def test_a_result_or_the_events_is_its_list(rec):
    scr = cj.ConjunctionResult(np.zeros(S), np.zeros(S, dtype=I32), np.zeros(S), PAIRS, 3)
    ev = np.zeros((3, 2, 4)); ev[:, 0] = PAIRS
    events = cj.EncounterEvents(ev, np.zeros((3, 2, 2), dtype=I32), np.ones(3, dtype=I32), np.zeros(3, dtype=I32))
    check_array(events.events, PAIRS, "events")
    assert cj.collision_probability(scr, 5.0, Y, UNITS, SPAN, P).pairs is PAIRS
    assert cj.screen_pairs(scr, T0, T1, eph=EPH)[0].shape == (3, 4)
    assert cj.collision_probability_window(events, 5.0, Y, UNITS, SPAN, P, 10.0).pairs is events.events
    assert cj.avoidance_window(events, 0.001, 5.0, Y, U, UNITS, SPAN, CONSTS, P, 10.0).pairs is events.events
    assert cj.avoidance_refine(events, 500.0, Y, U, UNITS, SPAN, CONSTS, M, T0, T1).pairs is events.events
    cj.screen_track(events, T0, T1, eph=EPH)
    assert [c[1][2] is (PAIRS if i < 2 else events.events) for i, c in enumerate(rec.calls)] == [True] * 6


def test_every_list_call_takes_the_events(rec):
    """an EncounterEvents offers its rows to collision_probability, avoidance, avoidance_joint, screen_pairs and screen_events
    (its own docstring): the library gets events.events"""
    ev = np.zeros((3, 2, 4)); ev[:, 0] = PAIRS
    events = cj.EncounterEvents(ev, np.zeros((3, 2, 2), dtype=I32), np.ones(3, dtype=I32), np.zeros(3, dtype=I32))
    assert cj.collision_probability(events, 5.0, Y, UNITS, SPAN, P).pairs is events.events
    assert cj.avoidance(events, 500.0, Y, U, UNITS, SPAN, CONSTS).pairs is events.events
    assert cj.avoidance_joint(events, 500.0, Y, U, UNITS, SPAN, CONSTS).pairs is events.events
    cj.screen_pairs(events, T0, T1, eph=EPH)
    cj.screen_events(events, T0, T1, eph=EPH)
    assert [c[0] for c in rec.calls] == ["mpcx_collision_probability", "mpcx_avoidance", "mpcx_avoidance_joint", "mpcx_conjunction_pairs",
                                         "mpcx_conjunction_events"]
    assert all(c[1][2] is events.events for c in rec.calls)
    rec.calls.clear()
    for f in LIST_CALLS:                                                # and one message says so everywhere
        with pytest.raises(ValueError) as e:
            call(f, pairs=np.zeros(3))
        assert str(e.value) == "pairs: expected (n, 4) rows (i, j, distance, time), a ConjunctionResult or an EncounterEvents, got (3,)", f
    assert rec.calls == []


# ------------------------------------------------------------------------------------------------ the messages of the shared checks
MESSAGES = [(f, dict(mu=0.0), "mu: need > 0 m^3/s^2, got 0.0") for f in ("collision_probability",) + WINDOW_CALLS[:1] + PLAN_CALLS]
MESSAGES += [(f, dict(max_step=0.0), "max_step: need > 0, got 0.0") for f in ("covariance", "covariance_thrust") + PLAN_CALLS]
MESSAGES += [(f, dict(half_window=[1.0, 2.0]), "half_window: expected a scalar or (3,) seconds, got (2,)") for f in WINDOW_CALLS]
MESSAGES += [(f, dict(half_window=None), "half_window: expected a scalar or (3,) seconds, got None") for f in WINDOW_CALLS]
MESSAGES += [(f, dict(panels=65), "panels: need an integer in 1 .. 64, got 65") for f in WINDOW_CALLS]
MESSAGES += [(f, dict(cat=CAT_RADII[:4]), "cat: expected (cat_Y, cat_units, cat_span, cat_P, cat_radius[, cat_ns]), got 4 items") for f in RADII_CAT]
MESSAGES += [(f, dict(cat=CAT_RADII[:5] + ([4.0] * 3,)), "cat_ns: expected (2,) node counts, got (3,)") for f in RADII_CAT]
MESSAGES += [(f, dict(cat=(CY, CUNITS, CSPAN, CP, [4.0] * 3)), "cat_radius: expected a scalar or (2,) hard-body radii in m, got (3,)") for f in RADII_CAT]
MESSAGES += [(f, dict(cat=(CY, CUNITS)), "cat: expected (cat_Y, cat_units, cat_span[, cat_P][, cat_ns]), got 2 items")
             for f in ("avoidance", "avoidance_joint", "avoidance_refine")]
MESSAGES += [(f, dict(cat=(CY, CUNITS, CSPAN, CP)), "P and cat_P come together (a Mahalanobis target) or not at all (a target in metres)")
             for f in ("avoidance", "avoidance_joint", "avoidance_refine")]
MESSAGES += [(f, dict(cat=(CY, CUNITS, CSPAN), P=P), "P and cat_P come together (a Mahalanobis target) or not at all (a target in metres)")
             for f in ("avoidance", "avoidance_joint", "avoidance_refine")]
MESSAGES += [(f, dict(q=[1.0, 2.0]), "q: expected a scalar or (3,) acceleration noise densities (m^2/s^3), got (2,)") for f in ("covariance", "covariance_thrust")]
MESSAGES += [(f, dict(q=-1.0), "q: need densities >= 0") for f in ("covariance", "covariance_thrust")]
MESSAGES += [("avoidance_window_refine", dict(recov=True, q=[1.0, 2.0]), "q: expected a scalar or (3,) acceleration noise densities (m^2/s^3), got (2,)")]
MESSAGES += [(f, dict(u_max=[1.0, 2.0]), "u_max: expected a scalar or (3,) normalised thrust limits, got (2,)") for f in ("avoidance_joint", "avoidance_refine")]
MESSAGES += [(f, dict(u_max=0.0), "u_max: need positive limits (inf: no ball)") for f in ("avoidance_joint", "avoidance_refine")]
MESSAGES += [(f, dict(rounds=-1), "rounds: need an integer >= 0, got -1") for f in ("avoidance_window_refine", "avoidance_refine")]
MESSAGES += [(f, dict(prop_max_step=0.0), "prop_max_step: need > 0, got 0.0") for f in ("avoidance_window_refine", "avoidance_refine")]
MESSAGES += [("avoidance_window_refine", dict(track=(M, T0)), f"track: expected None or (M, T0, T1), got {(M, T0)!r}"),
             ("avoidance_window_refine", dict(track=(1, T0, T1)), "M: need an integer >= 2 common instants, got 1"),
             ("avoidance_window_refine", dict(track=(M, T0, T1), max_shift=np.nan),
              "max_shift: need a number of seconds that is not NaN (None or <= 0: unlimited), got nan"),
             ("avoidance_refine", dict(track=True, max_shift=np.nan), "max_shift: need a number of seconds that is not NaN (None or <= 0: unlimited), got nan"),
             ("screen_track", dict(max_shift=[1.0]), "max_shift: need a number of seconds that is not NaN (None or <= 0: unlimited), got [1.0]"),
             ("avoidance_refine", dict(devices=[0, 0]),
              "devices: avoidance_refine runs on one device (every round needs every mover's new trajectory), got 2")]
MESSAGES += [(f, dict(target_p=1.0), "target_p: need a probability strictly between 0 and 1, got 1.0") for f in WINDOW_CALLS[2:]]
MESSAGES += [(f, dict(tol=0.0), "tol: need a positive finite number, got 0.0") for f in WINDOW_CALLS[2:] + ("avoidance_joint", "avoidance_refine")]
MESSAGES += [(f, dict(max_eval=0), "max_eval: need an integer >= 1, got 0") for f in WINDOW_CALLS[2:]]
MESSAGES += [(f, dict(who="k"), "who: expected 'i', 'j' or 'both', got 'k'") for f in ("avoidance",) + WINDOW_CALLS[1:]]
MESSAGES += [(f, dict(who="j", cat=CAT_RADII), "who = 'j': against a catalogue only the satellite can manoeuvre (who='i')") for f in WINDOW_CALLS[1:]]
MESSAGES += [("avoidance", dict(who="j", cat=CAT_PLAIN[:3]), "who = 'j': against a catalogue only the satellite can manoeuvre (who='i')")]
MESSAGES += [(f, dict(P=None), "P: the covariances at the nodes (covariance) are required") for f in WINDOW_CALLS[1:]]
MESSAGES += [(f, dict(P=P[:, :4]), "P: expected (3, 5, 6, 6) covariances at the nodes (covariance), got (3, 4, 6, 6)")
             for f in ("avoidance", "avoidance_joint", "avoidance_refine") + WINDOW_CALLS[1:]]
MESSAGES += [(f, dict(ns=[5, 5]), "ns: expected (3,) node counts, got (2,)") for f in PUBLIC]
MESSAGES += [(f, dict(U=U[:, :, :4]), "U: expected (3, 3, 5) thrust at the nodes, got (3, 3, 4)") for f in ("covariance", "covariance_thrust") + PLAN_CALLS]
MESSAGES += [(f, dict(consts=CONSTS[:, :7]), "consts: expected (3, 8) normalised constants per satellite, got (3, 7)")
             for f in ("covariance", "covariance_thrust") + PLAN_CALLS]
MESSAGES += [(f, dict(Y=Y[:, :, :1]), "Y: a covariance needs at least 2 nodes, got (3, 7, 1)") for f in ("covariance", "covariance_thrust")]
MESSAGES += [(f, dict(Y=Y[:, :, :1], U=U[:, :, :1], **({} if f in ("avoidance", "avoidance_joint", "avoidance_refine") else {"P": P[:, :1]})),
              "Y: need at least 2 nodes, got (3, 7, 1)") for f in PLAN_CALLS]
MESSAGES += [("covariance_thrust", dict(U=None), "U: covariance_thrust needs the thrust at the nodes (without thrust: covariance)"),
             ("covariance_thrust", dict(mass_var0=[1.0, 2.0]), "mass_var0: expected a scalar or (3,) values, got (2,)"),
             ("covariance_thrust", dict(execution=np.zeros(4)), "execution: expected (5,) or (3, 5) rows (s_fm, s_pm, s_fp, s_pp, u_off) (gates_execution), got (4,)"),
             ("covariance", dict(P0=np.zeros((2, 6, 6))), "P0: expected (6, 6) or (3, 6, 6) covariances of position (m) and velocity (m/s), got (2, 6, 6)")]
MESSAGES += [(f, dict(radius=[1.0, 2.0]), "radius: expected a scalar or (3,) hard-body radii in m, got (2,)") for f in RADII_CAT]
MESSAGES += [(f, dict(target=0.0), "target: need a positive finite distance, got 0.0") for f in ("avoidance", "avoidance_joint", "avoidance_refine")]


@pytest.mark.parametrize("f, kw, message", MESSAGES, ids=[f"{f}-{'-'.join(kw)}-{i}" for i, (f, kw, _) in enumerate(MESSAGES)])
def test_messages_of_the_shared_checks(rec, f, kw, message):
    with pytest.raises(ValueError) as e:
        call(f, **kw)
    assert str(e.value) == message
    assert rec.calls == []


# ------------------------------------------------------------------------------------------------ ConstellationMPC
CALLS = ("screen", "screen_against", "screen_events", "covariance", "covariance_thrust", "collision_probability", "collision_probability_window",
         "avoidance", "avoidance_window", "avoidance_window_refine", "avoidance_joint", "avoidance_refine", "cumulative_probability")


@pytest.fixture
def mpc(monkeypatch):
    """a ConstellationMPC with a hand-made plan whose every conjunction call is recorded as (name, args, kwargs) and returns a token"""
    from test_conjunction_host import hand_made_mpc
    m, _ = hand_made_mpc()
    m._plan = (ramp(3, 7, 6), ramp(3, 3, 6, start=1.0), np.zeros((3, 7, 6)))
    m.plan_K, m.plan_tf = np.array([6, 5, 4], dtype=np.int32), np.array([1.0, 0.9, 0.8])
    m.options = {"u_lim": [[0, 1.0], [0, 2.0], [0, 3.0]]}
    m.plan_drag, m.atmosphere, m.device, m.devices = True, ATMO, 1, [1, 2]
    m.calls = []

    class Token:
        def __init__(self, name):
            self.name, self.events, self.pc = name, name + ".events", name + ".pc"

    def recorder(name):
        def fn(*a, **kw):
            m.calls.append((name, a, kw))
            return Token(name)
        return fn
    for name in CALLS:
        monkeypatch.setattr(cj, name, recorder(name))
    return m


def window_of(m, samples_per_node=4):
    (w,) = m._screen_windows("plan", samples_per_node)
    return w


def same(a, b):
    """equal, arrays by content"""
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b)
    if isinstance(a, (tuple, list)) and isinstance(b, (tuple, list)):
        return type(a) is type(b) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict) and isinstance(b, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    return type(a) is type(b) and (a is b or a == b)


def check_mpc_calls(m, want):
    assert [c[0] for c in m.calls] == [w[0] for w in want]
    for (name, a, kw), (_, wa, wkw) in zip(m.calls, want):
        assert len(a) == len(wa), (name, len(a))
        for i, (x, y) in enumerate(zip(a, wa)):
            assert (x.name == y[1:] if isinstance(y, str) and y.startswith("@") else same(x, y)), (name, i, x, y)
        assert sorted(kw) == sorted(wkw), (name, sorted(kw), sorted(wkw))
        for k in kw:
            assert (kw[k].name == wkw[k][1:] if isinstance(wkw[k], str) and wkw[k].startswith("@") else same(kw[k], wkw[k])), (name, k, kw[k], wkw[k])


WHERE = dict(device=1, devices=[1, 2])
PLAN_MODEL = dict(include_drag=True, include_J2=False, atmosphere=ATMO)
TRUTH_MODEL = dict(include_drag=True, include_J2=True, atmosphere=ATMO)
MPC_CAT_RADII = (CY, CUNITS, CSPAN, CP, CRADIUS, CNS)


def screen_call(m, catalogue, threshold=1000.0, max_pairs=None, samples_per_node=4, cat_ns=CNS):
    w = window_of(m, samples_per_node)
    kw = dict(threshold=threshold, **WHERE, **w, **({} if max_pairs is None else {"max_pairs": max_pairs}))
    if catalogue:
        return ("screen_against", (), dict(kw, cat_Y=CY, cat_units=CUNITS, cat_span=CSPAN, cat_ns=cat_ns))
    return ("screen", (), kw)


def covariance_call(m, q=None, execution=None, mass_var0=None):
    w = window_of(m)
    if execution is None:
        return ("covariance", (w["Y"], w["units"], w["span"], m.consts, P0), dict(U=m._plan[1], ns=w["ns"], q=q, **PLAN_MODEL, **WHERE))
    return ("covariance_thrust", (w["Y"], w["units"], w["span"], m.consts, P0, m._plan[1], execution),
            dict(mass_var0=mass_var0, ns=w["ns"], q=q, **PLAN_MODEL, **WHERE))


def u_max_of(m):
    return f64([1.0, 2.0, 3.0])


@pytest.mark.parametrize("catalogue", [False, True])
def test_mpc_collision_probability(mpc, catalogue):
    w = window_of(mpc, 2)
    cat = MPC_CAT_RADII if catalogue else None
    ex = np.zeros(5)
    res = mpc.collision_probability(1000.0, P0, 5.0, q=0.5, samples_per_node=2, max_pairs=9, catalogue=cat, execution=ex, mass_var0=0.1)
    plan = (w["Y"], w["units"], w["span"])
    check_mpc_calls(mpc, [screen_call(mpc, catalogue, max_pairs=9, samples_per_node=2), covariance_call(mpc, 0.5, ex, 0.1),
                          ("collision_probability", ("@" + mpc.calls[0][0], 5.0, *plan, "@covariance_thrust"), dict(ns=w["ns"], cat=cat, **WHERE))])
    assert [r.name for r in res] == [mpc.calls[0][0], "collision_probability"]
    if catalogue:
        mpc.calls.clear()
        mpc.collision_probability(1000.0, P0, 5.0, catalogue=MPC_CAT_RADII[:5])
        check_mpc_calls(mpc, [screen_call(mpc, True, cat_ns=None), covariance_call(mpc),
                              ("collision_probability", ("@screen_against", 5.0, *window_plan(mpc), "@covariance"),
                               dict(ns=w["ns"], cat=MPC_CAT_RADII[:5], **WHERE))])


def window_plan(m):
    w = window_of(m)
    return (w["Y"], w["units"], w["span"])


@pytest.mark.parametrize("catalogue", [False, True])
def test_mpc_collision_probability_window(mpc, catalogue):
    w = window_of(mpc)
    cat = MPC_CAT_RADII if catalogue else None
    res = mpc.collision_probability_window(1000.0, P0, 5.0, 60.0, panels=3, catalogue=cat)
    scr = "@" + ("screen_against" if catalogue else "screen")
    plan = dict(ns=w["ns"], cat=cat, **WHERE)
    check_mpc_calls(mpc, [screen_call(mpc, catalogue), covariance_call(mpc),
                          ("collision_probability", (scr, 5.0, *window_plan(mpc), "@covariance"), plan),
                          ("collision_probability_window", (scr, 5.0, *window_plan(mpc), "@covariance", 60.0), dict(panels=3, **plan))])
    assert [r.name for r in res] == [scr[1:], "collision_probability", "collision_probability_window"]


@pytest.mark.parametrize("catalogue", [False, True])
def test_mpc_avoidance_window(mpc, catalogue):
    w = window_of(mpc)
    cat = MPC_CAT_RADII if catalogue else None
    res = mpc.avoidance_window(1000.0, P0, 5.0, 60.0, 0.001, q=0.5, catalogue=cat, who="i", tol=1e-4, max_eval=9)
    scr = "@" + ("screen_against" if catalogue else "screen")
    plan = dict(ns=w["ns"], cat=cat, **WHERE)
    check_mpc_calls(mpc, [screen_call(mpc, catalogue), covariance_call(mpc, 0.5),
                          ("collision_probability_window", (scr, 5.0, *window_plan(mpc), "@covariance", 60.0), dict(panels=4, **plan)),
                          ("avoidance_window", (scr, 0.001, 5.0, w["Y"], mpc._plan[1], w["units"], w["span"], mpc.consts, "@covariance", 60.0),
                           dict(panels=4, who="i", tol=1e-4, max_eval=9, **PLAN_MODEL, **plan))])
    assert [r.name for r in res] == [scr[1:], "collision_probability_window", "avoidance_window"]


@pytest.mark.parametrize("truth", [False, True])
@pytest.mark.parametrize("catalogue", [False, True])
def test_mpc_avoidance_window_refine(mpc, catalogue, truth):
    w = window_of(mpc)
    cat = MPC_CAT_RADII if catalogue else None
    res = mpc.avoidance_window_refine(1000.0, P0, 5.0, 60.0, 0.001, rounds=1, model="truth" if truth else "plan", q=0.5, catalogue=cat,
                                      track=not truth, max_shift=7.0)
    scr = "@" + ("screen_against" if catalogue else "screen")
    plan = dict(ns=w["ns"], cat=cat, **WHERE)
    check_mpc_calls(mpc, [screen_call(mpc, catalogue), covariance_call(mpc, 0.5),
                          ("collision_probability_window", (scr, 5.0, *window_plan(mpc), "@covariance", 60.0), dict(panels=4, **plan)),
                          ("avoidance_window_refine", (scr, 0.001, 5.0, w["Y"], mpc._plan[1], w["units"], w["span"], mpc.consts, "@covariance", 60.0),
                           dict(rounds=1, track=None if truth else (w["M"], w["T0"], w["T1"]), max_shift=7.0, recov=True, q=0.5, prop_max_step=1e-3,
                                panels=4, who="i", tol=_ffi.AW_DEFAULT_TOL, max_eval=_ffi.AW_DEFAULT_MAX_EVAL,
                                **(TRUTH_MODEL if truth else PLAN_MODEL), **plan))])
    assert [r.name for r in res] == [scr[1:], "collision_probability_window", "avoidance_window_refine"]


@pytest.mark.parametrize("catalogue", [False, True])
def test_mpc_encounters(mpc, catalogue):
    w = window_of(mpc)
    res = mpc.encounters(1000.0, max_events=3, catalogue=(CY, CUNITS, CSPAN, CNS) if catalogue else None)
    scr = "@" + ("screen_against" if catalogue else "screen")
    cat_kw = dict(cat_Y=CY, cat_units=CUNITS, cat_span=CSPAN, cat_ns=CNS) if catalogue else {}
    check_mpc_calls(mpc, [screen_call(mpc, catalogue, cat_ns=i32(CNS)), ("screen_events", (scr,), dict(threshold=1000.0, max_events=3, **w, **cat_kw, **WHERE))])
    assert [r.name for r in res] == [scr[1:], "screen_events"]
    mpc.calls.clear()
    cat = MPC_CAT_RADII if catalogue else None
    res = mpc.encounters(1000.0, P0=P0, radius_m=5.0, q=0.5, catalogue=cat)
    check_mpc_calls(mpc, [screen_call(mpc, catalogue, cat_ns=i32(CNS)), covariance_call(mpc, 0.5),
                          ("screen_events", (scr,), dict(threshold=1000.0, max_events=16, **w, **cat_kw, **WHERE)),
                          ("collision_probability", ("screen_events.events", 5.0, *window_plan(mpc), "@covariance"), dict(ns=w["ns"], cat=cat, **WHERE)),
                          ("cumulative_probability", ("@screen_events", "collision_probability.pc"), {})])
    assert [r.name for r in res] == [scr[1:], "screen_events", "collision_probability", "cumulative_probability"]


@pytest.mark.parametrize("catalogue", [None, (CY, CUNITS, CSPAN), (CY, CUNITS, CSPAN, CP, CNS)], ids=["inside", "catalogue", "catalogue P ns"])
def test_mpc_avoidance(mpc, catalogue):
    w = window_of(mpc)
    with_p = catalogue is None or len(catalogue) == 5
    res = mpc.avoidance(1000.0, 500.0, P0=P0 if with_p else None, q=0.5, catalogue=catalogue, who="i")
    scr = "@" + ("screen" if catalogue is None else "screen_against")
    want = [screen_call(mpc, catalogue is not None, cat_ns=i32(CNS) if catalogue is not None and len(catalogue) == 5 else None)]
    want += [covariance_call(mpc, 0.5)] if with_p else []
    want += [("avoidance", (scr, 500.0, w["Y"], mpc._plan[1], w["units"], w["span"], mpc.consts),
              dict(ns=w["ns"], P="@covariance" if with_p else None, cat=catalogue, who="i", **PLAN_MODEL, **WHERE))]
    check_mpc_calls(mpc, want)
    assert [r.name for r in res] == [scr[1:], "avoidance"]


@pytest.mark.parametrize("catalogue", [None, (CY, CUNITS, CSPAN, CNS)], ids=["inside", "catalogue"])
def test_mpc_avoidance_joint(mpc, catalogue):
    w = window_of(mpc)
    res = mpc.avoidance_joint(1000.0, 500.0, catalogue=catalogue, who="i", hold_terminal=False, tol=1e-8, max_iter=7, return_rows=True)
    scr = "@" + ("screen" if catalogue is None else "screen_against")
    check_mpc_calls(mpc, [screen_call(mpc, catalogue is not None, cat_ns=i32(CNS)),
                          ("avoidance_joint", (scr, 500.0, w["Y"], mpc._plan[1], w["units"], w["span"], mpc.consts),
                           dict(ns=w["ns"], P=None, cat=catalogue, who="i", u_max=u_max_of(mpc), hold_terminal=False, tol=1e-8, max_iter=7, return_rows=True,
                                return_terminal=False, **PLAN_MODEL, **WHERE))])
    assert mpc.calls[-1][2]["u_max"].flags.c_contiguous and [r.name for r in res] == [scr[1:], "avoidance_joint"]


@pytest.mark.parametrize("events", [False, True])
@pytest.mark.parametrize("catalogue", [None, (CY, CUNITS, CSPAN, CNS)], ids=["inside", "catalogue"])
def test_mpc_avoidance_refine(mpc, catalogue, events):
    w = window_of(mpc)
    res = mpc.avoidance_refine(1000.0, 500.0, rounds=1, P0=P0, q=0.5, catalogue=catalogue, model="truth" if events else "plan", events=events,
                               max_events=3, return_rhs=True)
    scr = "@" + ("screen" if catalogue is None else "screen_against")
    cat_kw = {} if catalogue is None else dict(cat_Y=CY, cat_units=CUNITS, cat_span=CSPAN, cat_ns=i32(CNS))
    want = [screen_call(mpc, catalogue is not None, cat_ns=i32(CNS)), covariance_call(mpc, 0.5)]
    want += [("screen_events", (scr,), dict(threshold=1000.0, max_events=3, **w, **cat_kw, **WHERE))] if events else []
    want += [("avoidance_refine", ("screen_events.events" if events else scr, 500.0, w["Y"], mpc._plan[1], w["units"], w["span"], mpc.consts, w["M"],
                                   w["T0"], w["T1"]),
              dict(track=events, rounds=1, ns=w["ns"], P="@covariance", cat=catalogue, who="i", u_max=u_max_of(mpc), hold_terminal=True,
                   tol=_ffi.AJ_DEFAULT_TOL, max_iter=_ffi.AJ_DEFAULT_MAX_ITER, prop_max_step=1e-3, return_rows=False, return_terminal=False,
                   return_rhs=True, device=1, devices=[1], **(TRUTH_MODEL if events else PLAN_MODEL)))]
    check_mpc_calls(mpc, want)
    assert [r.name for r in res] == [scr[1:]] + (["screen_events"] if events else []) + ["avoidance_refine"]


def test_mpc_catalogue_messages(mpc):
    radii = "catalogue: expected (Y, units, span, P, radius) or (Y, units, span, P, radius, ns), got 4 items"
    bad = (CY, CUNITS, CSPAN, CP)
    for call in (lambda: mpc.collision_probability(1000.0, P0, 5.0, catalogue=bad), lambda: mpc.collision_probability_window(1000.0, P0, 5.0, 60.0, catalogue=bad),
                 lambda: mpc.avoidance_window(1000.0, P0, 5.0, 60.0, 0.001, catalogue=bad),
                 lambda: mpc.avoidance_window_refine(1000.0, P0, 5.0, 60.0, 0.001, catalogue=bad)):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == radii
    for call in (lambda: mpc.avoidance(1000.0, 500.0, catalogue=(CY, CUNITS)), lambda: mpc.avoidance_joint(1000.0, 500.0, catalogue=(CY, CUNITS)),
                 lambda: mpc.avoidance_refine(1000.0, 500.0, catalogue=(CY, CUNITS))):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == "catalogue: expected (Y, units, span[, P][, ns]), got 2 items"
    with pytest.raises(ValueError) as e:
        mpc.screen_against((CY, CUNITS), 1000.0, what="plan")
    assert str(e.value) == "catalogue: expected (Y, units, span) or (Y, units, span, ns), got 2 items"
    assert [c[0] for c in mpc.calls] == []
