"""The listed-pair entry points of include/mpcx.h called through the C ABI by argument NAME, in their host-pointer and their _dev
form, on small real scenes: what tests/test_encounter_dev_forms_gpu.py, tests/test_encounter_host_messages_gpu.py and
tests/golden/make_encounter_host_messages.py share.

A call is a dict {argument name: value} -- numpy arrays, scalars, None for a NULL pointer; keys the entry point does not have are
ignored, so one scene serves many calls.  The order of the arguments is read from the header; their C types are _ffi._SIGS's.
The scenes are the stored inputs of tests/golden/encounter_parent_bits.npz (make_encounter_parent_bits.py says what they are)."""
import ctypes as C
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "include", "mpcx.h")
_names = {}


def argument_names(name):
    """the argument names of entry point `name` in the header's order, without ctx"""
    if not _names:
        text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
        text = re.sub(r"//[^\n]*", "", text)
        for m in re.finditer(r"\b(mpcx_\w+)\s*\(([^)]*)\)\s*;", text):
            _names[m.group(1)] = [re.split(r"[\s*]+", a.strip())[-1] for a in m.group(2).split(",")]
    return _names[name][1:]


def _env():
    from mpconstellation_amd import _ffi
    return _ffi, _ffi.load(), _ffi.context(0)


def last_error():
    _, lib, ctx = _env()
    return lib.mpcx_last_error(ctx).decode()


def _invoke(name, call, pointer):
    _ffi, lib, ctx = _env()
    types = _ffi._SIGS[name][1][1:]
    names = argument_names(name)
    assert len(types) == len(names), name
    return getattr(lib, name)(ctx, *[pointer(call[k], t) if t in (_ffi._dp, _ffi._ip, _ffi._lp, _ffi._vp) else call[k] for k, t in zip(names, types)])


def call_host(name, call):
    """the host-pointer form of `name` -> its return code"""
    def pointer(a, t):
        if a is None:
            return None
        assert a.flags.c_contiguous and a.dtype == {C.c_double: np.float64, C.c_int32: np.int32, C.c_int64: np.int64}[t._type_], (name, a.dtype)
        return a.ctypes.data_as(t)
    return _invoke(name, call, pointer)


def call_dev(name, call):
    """the _dev form of `name`: every array a torch tensor on the device, call["workspace"] too where the call has one (None: NULL),
    on torch's current stream -> its return code.  The caller synchronises."""
    import torch
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return _invoke(name + "_dev", dict(call, stream=stream), lambda a, t: a if a is stream else C.c_void_p(0 if a is None else a.data_ptr()))


def on_device(call):
    """the call with its arrays copied to device tensors"""
    import torch
    return {k: torch.tensor(v, device="cuda:0") if isinstance(v, np.ndarray) else v for k, v in call.items()}


def workspace_bytes(name, call):
    """bytes of the _dev form's workspace; 0 for a call that has none"""
    _, lib, _ = _env()
    fn = name.replace("_batch", "").replace("_tracked", "") + "_workspace_bytes"
    if "workspace" not in argument_names(name + "_dev"):
        return 0
    return int(getattr(lib, fn)(*[int(call[k]) for k in _names[fn]]))               # (a size function has no ctx: every name counts)


# ---------------------------------------------------------------- scenes
def parent_inputs(case):
    import sys
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_encounter_parent_bits as M
    return M.inputs_of(np.load(os.path.join(HERE, "golden", M.NAME)), case)


def _geometry(pairs, rows, cat):
    """the list and its two sides: rows = (Y, units, span, P, radius), cat the same five or None"""
    from mpconstellation_amd.constants import MU_EARTH
    names = ("Y", "units", "span", "P", "radius")
    g = dict(n=len(pairs), pairs=np.ascontiguousarray(pairs), S=len(rows[0]), K=rows[0].shape[2], Ks=None, mu=MU_EARTH,
             **{k: None if a is None else np.ascontiguousarray(a) for k, a in zip(names, rows)})
    g.update(D=0, cat_K=0, cat_Ks=None, **{"cat_" + k: None for k in names})
    if cat is not None:
        g.update(D=len(cat[0]), cat_K=cat[0].shape[2], **{"cat_" + k: None if a is None else np.ascontiguousarray(a) for k, a in zip(names, cat)})
    return g


def _plan(g, U, consts):
    from mpconstellation_amd import conjunction as cj
    return dict(g, U=np.ascontiguousarray(U), consts=np.ascontiguousarray(consts), flags=0, max_step=float(cj.DEFAULT_MAX_STEP))


def slow_pair(form):
    """the `figures` scene: the slow pair as a pair of one constellation ("pair") or as satellite against catalogue ("cat"), with its
    zero plan, one window of 2000 s and two panels"""
    w = parent_inputs("figures")
    five = tuple(w[k] for k in ("Y", "units", "span", "P", "radius"))
    if form == "pair":
        g = _geometry(w["pairs"], five, None)
    else:
        g = _geometry(np.array([[0.0, 0.0, 50.0, 3000.0]]), tuple(a[:1] for a in five), tuple(a[1:] for a in five))
    S, K = g["S"], g["K"]
    return dict(_plan(g, np.zeros((S, 3, K)), w["consts"][:S]), half_window=np.full(g["n"], 2000.0), panels=2, who=0,
                P0=np.ascontiguousarray(w["P"][:S, 0]), cat_consts=None if form == "pair" else np.ascontiguousarray(w["consts"][1:]),
                cat_P0=None if form == "pair" else np.ascontiguousarray(w["P"][1:, 0]))


def three_satellites(covariances=False):
    """the `loops` scene of the joint manoeuvre: three satellites against a catalogue, listed rows that share one"""
    w = parent_inputs("loops")
    S, _, K = w["fY"].shape
    P = np.ascontiguousarray(np.broadcast_to(np.eye(6) * 1e4, (S, K, 6, 6))) if covariances else None
    g = _geometry(w["fpairs"], (w["fY"], w["funits"], w["fspan"], P, None), (w["fcY"], w["fcunits"], w["fcspan"], P, None))
    g["cat_Ks"] = np.ascontiguousarray(w["fcns"])
    return dict(_plan(g, w["fU"], w["fconsts"]), mover=None, target=1.0e7 if P is None else 4.0, u_max=None, hold_terminal=0, tol=1e-10,
                max_iter=50, sat0=0, nsat=S)


# ---------------------------------------------------------------- results
F, I, L = np.float64, np.int32, np.int64


def results_of(name, c):
    """{result name: (shape, dtype, optional)} of call `name` on the scene / call `c`"""
    _ffi, _, _ = _env()
    n, S, K = c["n"], c["S"], c.get("K", 0)                               # (the list calls on an ephemeris have no K)
    NS = 1 if c.get("cat_Y") is not None else 2
    np_ = c.get("rounds", 0) + 2
    return {
        "mpcx_collision_probability": dict(out=((n, _ffi.NPC), F, 0), status=((n,), I, 0)),
        "mpcx_collision_probability_window": dict(out=((n, _ffi.NPW), F, 0), status=((n,), I, 0)),
        "mpcx_encounter_window": dict(out=((n, _ffi.NEW), F, 0), flags=((n,), I, 0), status=((n,), I, 0)),
        "mpcx_collision_window_sensitivity": dict(out=((n, _ffi.NPW), F, 0), sens=((n, NS, 3, K), F, 0),
                                                  state_grad=((n, 64 * c.get("panels", 1) + 1, 6), F, 1), status=((n,), I, 0)),
        "mpcx_avoidance": dict(out=((n, _ffi.NAV), F, 0), du=((n, NS, 3, K), F, 0), sens=((n, NS, 9, K), F, 1), status=((n,), I, 0)),
        "mpcx_avoidance_window": dict(out=((n, _ffi.NAW), F, 0), du=((n, NS, 3, K), F, 0), sens=((n, NS, 3, K), F, 1), status=((n,), I, 0)),
        "mpcx_avoidance_window_refine": dict(out=((n, _ffi.NAW), F, 0), du=((n, NS, 3, K), F, 0), sens=((n, NS, 3, K), F, 1), status=((n,), I, 0),
                                             rounds_done=((n,), I, 0), Y_out=((n * NS, 7, K), F, 0), P_out=((n * NS, K, 6, 6), F, 1),
                                             hist_p=((np_, n), F, 0), hist_t=((np_, n), F, 0), hist_pred=((np_ - 1, n), F, 0)),
        "mpcx_avoidance_joint": dict(du=((S, 3, K), F, 0), sat_out=((S, _ffi.NAJ), F, 0), row_out=((n, _ffi.NAR), F, 0), rows=((n, 3, K), F, 1),
                                     tsens=((S, 18, K), F, 1), sat_status=((S,), I, 0), row_status=((n,), I, 0)),
        "mpcx_avoidance_refine": dict(du=((S, 3, K), F, 0), sat_out=((S, _ffi.NAJ), F, 0), row_out=((n, _ffi.NAR), F, 0), rows=((n, 3, K), F, 1),
                                      tsens=((S, 18, K), F, 1), sat_status=((S,), I, 0), row_status=((n,), I, 0), Y_out=((S, 7, K), F, 0),
                                      pairs_out=((n, 4), F, 0), hist_d0=((np_, n), F, 0), hist_tca=((np_, n), F, 0), hist_term=((np_, S), F, 0),
                                      rounds_done=((S,), I, 0), rhs_rows=((n,), F, 1), rhs_term=((S, 6), F, 1)),
        "mpcx_collision_probability_mc": dict(counts=((n, _ffi.NMCC), L, 0), out=((n, _ffi.NMC), F, 0), status=((n,), I, 0),
                                              samples=((n, c.get("n_samples", 1), _ffi.NMS), F, 1)),
        "mpcx_covariance_batch": dict(P=((S, K, 6, 6), F, 0), status=((S,), I, 0)),
        "mpcx_covariance_thrust_batch": dict(P=((S, K, 6, 6), F, 0), Pm=((S, K, 7), F, 1), status=((S,), I, 0)),
        "mpcx_conjunction_pairs": dict(out=((n, 4), F, 0), status=((n,), I, 0)),
        "mpcx_conjunction_events": dict(events=((n, c.get("max_events", 1), 4), F, 0), info=((n, c.get("max_events", 1), 2), I, 0),
                                        count=((n,), I, 0), status=((n,), I, 0)),
        "mpcx_conjunction_track": dict(out=((n, 4), F, 0), info=((n, 2), I, 1), status=((n,), I, 0)),
    }[name.replace("_tracked", "")]


def with_results(name, c, optional=True):
    """the call with fresh host arrays for its results (the optional ones too, or NULL)"""
    return dict(c, **{k: np.zeros(shape, dtype=dt) if optional or not opt else None for k, (shape, dt, opt) in results_of(name, c).items()})


# ---------------------------------------------------------------- one valid small call of every entry point of the family
def _covariance_call():
    w = parent_inputs("covariance")
    units = w["units"].copy()
    units[3, 1] = units[2, 1]                                            # (the stored case has a zero time unit on purpose)
    S, _, K = w["Y"].shape
    return dict(S=S, K=K, Ks=np.ascontiguousarray(w["ns"]), X=w["Y"], U=w["U"], units=units, span=w["span"], consts=w["consts"], flags=0,
                max_step=1e-2, P0=np.ascontiguousarray(np.broadcast_to(w["P0"], (S, 6, 6))), q=None, exec=np.zeros((S, 5)), m_var0=None, n=S)


def _list_call():
    """three satellites against two catalogue objects on a common clock of M instants: any finite ephemeris is a valid one"""
    S, D, M = 3, 2, 9
    rng = np.random.default_rng(5)
    eph, cat = 7.0e6 * rng.standard_normal((S, 6, M)), 7.0e6 * rng.standard_normal((D, 6, M))
    return dict(n=2, pairs=np.array([[0.0, 1.0, 0.0, 300.0], [2.0, 0.0, 0.0, 500.0]]), S=S, D=D, M=M, eph=eph, cat=cat, T0=0.0, T1=800.0,
                threshold=1.0e9, max_events=3, max_shift=100.0)


BASE = {
    "mpcx_collision_probability": lambda: slow_pair("cat"),
    "mpcx_collision_probability_window": lambda: slow_pair("cat"),
    "mpcx_collision_window_sensitivity": lambda: slow_pair("cat"),
    "mpcx_encounter_window": lambda: dict(slow_pair("cat"), max_half=np.full(1, 2000.0), nsigma=8.0, levels=3),
    "mpcx_collision_probability_mc": lambda: dict(slow_pair("cat"), prop_max_step=1e-3, exec=None, m_var0=None, scan=8, n_samples=8, seed=1,
                                                  max_flights=0, Y_samples=None, U_samples=None),
    "mpcx_avoidance": lambda: dict(slow_pair("cat"), target=4.0),
    "mpcx_avoidance_window": lambda: dict(slow_pair("cat"), target_p=1e-3, tol=1e-6, max_eval=40),
    "mpcx_avoidance_window_refine": lambda: dict(slow_pair("cat"), target_p=1e-3, tol=1e-6, max_eval=40, prop_max_step=1e-3, rounds=1, M=0, T0=0.0,
                                                 T1=1.0, max_shift=0.0, recov=0, q=None),
    "mpcx_avoidance_joint": lambda: three_satellites(True),
    "mpcx_avoidance_refine": lambda: dict(three_satellites(True), M=17, T0=-1.0, T1=2999.0, prop_max_step=1e-3, rounds=1),
    "mpcx_avoidance_refine_tracked": lambda: dict(three_satellites(True), M=17, T0=-1.0, T1=2999.0, prop_max_step=1e-3, rounds=1, max_shift=400.0),
    "mpcx_covariance_batch": _covariance_call,
    "mpcx_covariance_thrust_batch": _covariance_call,
    "mpcx_conjunction_pairs": _list_call,
    "mpcx_conjunction_events": _list_call,
    "mpcx_conjunction_track": _list_call,
}


def base_call(name):
    """a valid small call of `name`, every result given"""
    return with_results(name, BASE[name]())
