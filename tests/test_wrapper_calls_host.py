"""What the batched Python wrappers hand to libmpcx.so, pinned call by call without a device: _ffi.load / _ffi.context are
replaced by a recorder, _ffi.dptr / _ffi.iptr return the array itself, and every scenario checks the entry point's name, the
argument count against _ffi._SIGS, every scalar, and dtype / contiguity / shape / contents of every array (None where the
C signature takes NULL).  Output buffers are checked for dtype, contiguity and shape, and for their contents where the
wrapper defines them (zeroed status words, the held final times).  Nothing is solved."""
import numpy as np
import pytest

from mpconstellation_amd import _ffi
from mpconstellation_amd.optimizer import (constraint_terms_batch, mpc_step_batch, mpc_update_batch, scp_iteration_batch,
                                           solve_batch)
from mpconstellation_amd.simulator import propagate_batch

K = 5
I32 = np.int32


class Recorder:
    """stands in for the loaded library: every mpcx_* attribute records (name, args) and returns 0; mpcx_default_solve_opts
    is the real one.  `on[name]`, if set, is called with the arguments (to play the library writing a result)."""

    def __init__(self, real):
        self.real, self.calls, self.on = real, [], {}

    def __getattr__(self, name):
        if not name.startswith("mpcx_"):
            raise AttributeError(name)
        if name == "mpcx_default_solve_opts":
            return getattr(self.real, name)

        def fn(*args):
            self.calls.append((name, args))
            if name in self.on:
                self.on[name](*args)
            return 0
        return fn

    def named(self, *names):
        """the recorded calls of these entry points, in context-slot order (the blocks of a multi-device call run on threads)"""
        return sorted((c for c in self.calls if c[0] in names), key=lambda c: c[1][0][2])


@pytest.fixture
def rec(monkeypatch):
    from mpconstellation_amd import build
    build.build()                                       # (cross-compiles without a GPU, as in test_cabi.py; no-op when built)
    r = Recorder(_ffi.load())
    monkeypatch.setattr(_ffi, "load", lambda: r)
    monkeypatch.setattr(_ffi, "context", lambda device=0, slot=0: ("ctx", int(device), int(slot)))
    monkeypatch.setattr(_ffi, "dptr", lambda a: a)
    monkeypatch.setattr(_ffi, "iptr", lambda a: a)
    return r


class Out:
    """an output buffer: dtype, C-contiguity and shape; zero=True: handed over zeroed"""

    def __init__(self, *shape, dtype=np.float64, zero=False):
        self.shape, self.dtype, self.zero = shape, np.dtype(dtype), zero


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def i32(a):
    return np.ascontiguousarray(a, dtype=I32)


def check_array(a, want, what):
    assert isinstance(a, np.ndarray), what
    assert a.dtype == want.dtype and a.flags.c_contiguous and a.shape == want.shape, (what, a.dtype, a.shape, a.flags.c_contiguous)
    assert np.array_equal(a, want), (what, a, want)


def check_call(call, name, want):
    got, args = call
    assert got == name
    assert len(args) == len(_ffi._SIGS[name][1]), (name, len(args))
    assert len(want) == len(args), (name, len(want))
    for i, (a, w) in enumerate(zip(args, want)):
        what = f"{name} argument {i}"
        if w is None:
            assert a is None, what
        elif isinstance(w, Out):
            assert isinstance(a, np.ndarray) and a.dtype == w.dtype and a.flags.c_contiguous and a.shape == w.shape, (what, a)
            assert not w.zero or not a.any(), what
        elif isinstance(w, _ffi.SolveOpts):
            for field, _ in _ffi.SolveOpts._fields_:
                assert getattr(a._obj, field) == getattr(w, field), (what, field)
        elif isinstance(w, np.ndarray):
            check_array(a, w, what)
        elif isinstance(w, int):
            assert type(a) is int and a == w, (what, a, w)
        elif isinstance(w, float):
            assert isinstance(a, float) and a == w, (what, a, w)
        else:
            assert a == w, (what, a, w)
    return args


def step_inputs(S):
    xbar = np.arange(S * 7 * K, dtype=np.float64).reshape(S, 7, K)
    ubar = np.zeros((S, 3, K))
    consts = np.arange(S * 8, dtype=np.float64).reshape(S, 8)
    return xbar, ubar, consts


def step_outputs(S, tf=None):
    return [Out(S, 7, K), Out(S, 3, K), Out(S, 7, K), Out(S) if tf is None else tf, Out(S, dtype=I32, zero=True),
            Out(S, dtype=I32, zero=True), Out(S)]


CTX = ("ctx", 0, 0)
TABLE_OPTIONS = {"tf_max": [2.0, 3.0, 4.0], "u_lim": [[0, 1.0], [0, 2.0], [0, 3.0]], "eps_r": 0.02}
TABLE_FIRST = {"tf_max": 2.0, "u_lim": [0, 1.0], "eps_r": 0.02}          # the first satellite's values: what the struct carries


def result_is(res, args, first):
    """the SolveResult hands back the very arrays the library was given (X, U, NU, tf, status, iters, kkt from `first` on)"""
    for name, a in zip(("X", "U", "NU", "tf", "status", "iters", "kkt"), args[first:first + 7]):
        assert getattr(res, name) is a, name


# ------------------------------------------------------------------------------------------------ mpc_step_batch
def test_step_scalar_options_looks_the_entry_point_up_at_call_time_and_copies_nothing(rec):
    xbar, ubar, consts = step_inputs(3)
    inner = rec.mpcx_mpc_step_batch
    timed = []

    def swapped(*a):                                     # bench.py times the calls by replacing the attribute after import
        timed.append(a)
        return inner(*a)
    rec.mpcx_mpc_step_batch = swapped
    res = mpc_step_batch(xbar, ubar, 1.5, consts, 2.0, max_step=0.02)
    assert len(timed) == 1 and len(rec.calls) == 1
    args = check_call(rec.calls[0], "mpcx_mpc_step_batch",
                      [CTX, 3, K, xbar, ubar, np.full(3, 1.5), consts, np.full(3, 2.0), 0, 0.02, _ffi.make_solve_opts()] + step_outputs(3))
    assert args[3] is xbar and args[4] is ubar and args[6] is consts          # contiguous float64 goes through as it is
    result_is(res, args, 11)
    assert res.g_tf is None and res.n_regularised is None


def test_step_with_node_counts_is_the_ragged_call(rec):
    xbar, ubar, consts = step_inputs(3)
    res = mpc_step_batch(xbar, ubar, [1.0, 2.0, 3.0], consts, [1.0, 1.1, 1.2], Ks=[5, 4, 3], linear_vt=True, device=2, slot=1, tol=1e-6)
    args = check_call(rec.calls[0], "mpcx_mpc_step_batch_ragged",
                      [("ctx", 2, 1), 3, K, i32([5, 4, 3]), xbar, ubar, f64([1.0, 2.0, 3.0]), consts, f64([1.0, 1.1, 1.2]), 0, 1e-2,
                       _ffi.make_solve_opts(tol=1e-6, flags=_ffi.SOLVE_LINEAR_VT)] + step_outputs(3))
    result_is(res, args, 12)
    assert len(rec.calls) == 1


@pytest.mark.parametrize("Ks", [None, 4])
def test_step_with_a_per_satellite_option_is_the_table_call(rec, Ks):
    xbar, ubar, consts = step_inputs(3)
    res = mpc_step_batch(xbar, ubar, 1.0, consts, 1.0, TABLE_OPTIONS, Ks=Ks)
    table = _ffi.make_popts(TABLE_OPTIONS, 3)
    assert table.shape == (3, _ffi.NPOPT)
    args = check_call(rec.calls[0], "mpcx_mpc_step_batch_ragged_sat",
                      [CTX, 3, K, None if Ks is None else i32([4, 4, 4]), xbar, ubar, np.ones(3), consts, np.ones(3), 0, 1e-2,
                       _ffi.make_solve_opts(TABLE_FIRST), table] + step_outputs(3))
    o = args[11]._obj
    assert (o.tf_max, o.u_max, o.eps_r) == (2.0, 1.0, 0.02)
    result_is(res, args, 13)


def test_step_flag_word(rec):
    xbar, ubar, consts = step_inputs(3)
    mpc_step_batch(xbar, ubar, 1.0, consts, 1.0, include_drag=True, include_J2=True, uniform_steps=7, rk23=True)
    assert rec.calls[0][1][8] == 1 | 2 | 4 | 8 | 7 << 8 and type(rec.calls[0][1][8]) is int
    mpc_step_batch(xbar, ubar, 1.0, consts, 1.0, include_J2=True)
    assert rec.calls[1][1][8] == 2
    assert [c[0] for c in rec.calls] == ["mpcx_mpc_step_batch"] * 2


def test_step_fixed_tf_holds_the_values_on_entry(rec):
    xbar, ubar, consts = step_inputs(3)
    res = mpc_step_batch(xbar, ubar, 1.0, consts, 1.0, fixed_tf=[1.0, 2.0, 3.0], regularised=True)
    args = check_call(rec.calls[0], "mpcx_mpc_step_batch",
                      [CTX, 3, K, xbar, ubar, np.ones(3), consts, np.ones(3), 0, 1e-2, _ffi.make_solve_opts(flags=_ffi.SOLVE_FIXED_TF)]
                      + step_outputs(3, tf=f64([1.0, 2.0, 3.0])))
    assert res.g_tf is args[14] and res.tf is not args[14]
    check_array(res.tf, f64([1.0, 2.0, 3.0]), "held tf")
    reg = check_call(rec.calls[1], "mpcx_solve_regularised", [CTX, 3, Out(3, 2, dtype=I32, zero=True)])[2]
    assert np.shares_memory(res.n_regularised, reg) and np.shares_memory(res.first_regularised, reg)
    assert len(rec.calls) == 2


def test_step_shared_tf_refuses_a_table_before_any_call(rec):
    xbar, ubar, consts = step_inputs(3)
    with pytest.raises(ValueError):
        mpc_step_batch(xbar, ubar, 1.0, consts, 1.0, TABLE_OPTIONS, shared_tf=True)
    assert rec.calls == []
    mpc_step_batch(xbar, ubar, 1.0, consts, 1.0, shared_tf=True)
    assert rec.calls[0][0] == "mpcx_mpc_step_batch" and rec.calls[0][1][10]._obj.flags == _ffi.SOLVE_SHARED_TF


@pytest.mark.parametrize("table", [False, True])
def test_step_on_three_contexts_writes_one_result_set_in_place(rec, table):
    S = 8
    xbar, ubar, consts = step_inputs(S)
    r_des = 1.0 + np.arange(S)
    options = {"tf_max": 2.0 + np.arange(S), "eps_r": 0.02} if table else {"eps_r": 0.02}
    first_sat = {"tf_max": 2.0, "eps_r": 0.02} if table else options
    popts = _ffi.make_popts(options, S)
    res = mpc_step_batch(xbar, ubar, 1.5, consts, r_des, options, devices=[0, 0, 0], regularised=True, include_J2=True)
    name = "mpcx_mpc_step_batch_ragged_sat" if table else "mpcx_mpc_step_batch"
    calls = rec.named(name)
    regs = rec.named("mpcx_solve_regularised")
    assert len(calls) == 3 and len(regs) == 3 and len(rec.calls) == 6
    whole = (res.X, res.U, res.NU, res.tf, res.status, res.iters, res.kkt)
    for slot, (first, n) in enumerate([(0, 3), (3, 3), (6, 2)]):
        blk = slice(first, first + n)
        want = [("ctx", 0, slot), n, K] + ([None] if table else []) + \
               [xbar[blk], ubar[blk], np.full(n, 1.5), consts[blk], r_des[blk], 2, 1e-2, _ffi.make_solve_opts(first_sat)] + \
               ([popts[blk]] if table else []) + \
               [Out(n, 7, K), Out(n, 3, K), Out(n, 7, K), Out(n), Out(n, dtype=I32, zero=True), Out(n, dtype=I32, zero=True), Out(n)]
        args = check_call(calls[slot], name, want)
        for a, w in zip(args[-7:], whole):
            assert np.shares_memory(a, w) and a.ctypes.data == w[blk].ctypes.data
        reg = check_call(regs[slot], "mpcx_solve_regularised", [("ctx", 0, slot), n, Out(n, 2, dtype=I32, zero=True)])[2]
        assert np.shares_memory(reg, res.n_regularised) and reg.ctypes.data == res.n_regularised[blk].ctypes.data
        assert rec.calls.index(regs[slot]) > rec.calls.index(calls[slot])
    assert res.X.shape == (S, 7, K) and res.n_regularised.shape == (S,) and res.first_regularised.shape == (S,)


def test_step_on_several_contexts_refuses_fixed_and_shared_tf(rec):
    xbar, ubar, consts = step_inputs(3)
    for kw in (dict(fixed_tf=1.0), dict(shared_tf=True)):
        with pytest.raises(ValueError):
            mpc_step_batch(xbar, ubar, 1.0, consts, 1.0, devices=[0, 0], **kw)
    assert rec.calls == []
    mpc_step_batch(xbar, ubar, 1.0, consts, 1.0, devices=[3], fixed_tf=1.0)             # one device: the single-context call
    assert rec.calls[0][1][0] == ("ctx", 3, 0)


# ------------------------------------------------------------------------------------------------ mpc_update_batch
def update_want(ctx, S, n_scp, base_res, y0, horizon, consts, r_des, ref_thrust, prop_max_step, flags, max_step, opts, popts, sim, n_sim,
                records_zero=True):
    return [ctx, S, K, n_scp, base_res, y0, horizon, consts, r_des, ref_thrust, prop_max_step, flags, max_step, opts] + \
           ([] if popts is None else [popts]) + \
           [Out(S, 7, K), Out(S, 3, K), Out(S, 7, K), Out(S), Out(S, dtype=I32, zero=True), Out(n_scp, S, dtype=I32, zero=records_zero),
            Out(n_scp, S, dtype=I32, zero=records_zero), Out(S), Out(S, dtype=I32, zero=True)] + list(sim) + \
           [None if n_sim is None else Out(S, 7, n_sim), None if n_sim is None else Out(S, dtype=I32, zero=True)]


def update_inputs(S):
    return np.arange(S * 7, dtype=np.float64).reshape(S, 7), np.arange(S * 8, dtype=np.float64).reshape(S, 8)


NO_FLIGHT = (0.0, 0.0, 0, 0, 1e-3)


@pytest.mark.parametrize("table", [False, True])
def test_update_plain_and_table(rec, table):
    y0, consts = update_inputs(3)
    options = TABLE_OPTIONS if table else {"eps_r": 0.02}
    res = mpc_update_batch(y0, 2.0, consts, 1.5, 2.5, n_scp=3, options=options, ref_thrust=0.25, max_step=0.02, prop_max_step=2e-3,
                           include_J2=True, linear_vt=True, max_iter=77)
    name = "mpcx_mpc_update_batch_sat" if table else "mpcx_mpc_update_batch"
    opts = _ffi.make_solve_opts(TABLE_FIRST if table else options, max_iter=77, flags=_ffi.SOLVE_LINEAR_VT)
    args = check_call(rec.calls[0], name, update_want(CTX, 3, 3, 2.5, y0, np.full(3, 2.0), consts, np.full(3, 1.5), 0.25, 2e-3, 2, 0.02, opts,
                                                      _ffi.make_popts(options, 3), NO_FLIGHT, None))
    assert args[5] is y0 and args[7] is consts and len(rec.calls) == 1
    o = 15 if table else 14
    for name, a in zip(("X", "U", "NU", "tf", "Ks", "status", "iters", "kkt", "prop_status"), args[o:o + 9]):
        assert getattr(res, name) is a, name
    assert res.y_sim is None and res.sim_status is None


@pytest.mark.parametrize("fly, sim", [((0.5, 0.25, 4, True, False), (0.5, 0.25, 4, 1, 1e-3)),
                                      ((1, 2, 4, False, True, 5e-4), (1.0, 2.0, 4, 2, 5e-4)),
                                      ((0.5, 0.25, 4, 1, 1), (0.5, 0.25, 4, 3, 1e-3))])
def test_update_flight_segment(rec, fly, sim):
    y0, consts = update_inputs(3)
    res = mpc_update_batch(y0, [2.0, 2.0, 2.0], consts, [1.0, 2.0, 3.0], 2.5, fly=fly, include_drag=True, rollout_model=True, device=1)
    args = check_call(rec.calls[0], "mpcx_mpc_update_batch",
                      update_want(("ctx", 1, 0), 3, 2, 2.5, y0, np.full(3, 2.0), consts, f64([1.0, 2.0, 3.0]), 0.5, 1e-3, 1 | 16, 1e-2,
                                  _ffi.make_solve_opts(), None, sim, 4))
    assert res.y_sim is args[-2] and res.sim_status is args[-1]


def test_update_flags_and_horizon(rec):
    y0, consts = update_inputs(3)
    mpc_update_batch(y0, 2.0, consts, 1.0, 2.5, rollout_model=True)
    mpc_update_batch(y0, 2.0, consts, 1.0, 2.5, include_drag=True, include_J2=True)
    assert [c[1][11] for c in rec.calls] == [16, 3]
    with pytest.raises(ValueError):
        mpc_update_batch(y0, [2.0, 2.0, 2.5], consts, 1.0, 2.5)
    assert len(rec.calls) == 2


@pytest.mark.parametrize("table", [False, True])
def test_update_on_two_contexts_brings_the_iteration_records_back(rec, table):
    y0, consts = update_inputs(3)
    options = TABLE_OPTIONS if table else None
    popts = _ffi.make_popts(options, 3)
    name = "mpcx_mpc_update_batch_sat" if table else "mpcx_mpc_update_batch"
    st = 20 if table else 19                                  # status; iters follows

    def library_writes(*a):                                   # a block's columns of (n_scp, S) are not contiguous in the result set
        slot = a[0][2]
        a[st][...] = 100 * (slot + 1) + np.arange(a[st].size).reshape(a[st].shape)
        a[st + 1][...] = 1000 * (slot + 1) + np.arange(a[st].size).reshape(a[st].shape)
    rec.on[name] = library_writes
    r_des = f64([1.0, 2.0, 3.0])
    res = mpc_update_batch(y0, 2.0, consts, r_des, 2.5, n_scp=2, options=options, fly=(0.5, 0.25, 4, True, True), devices=[0, 0])
    calls = rec.named(name)
    assert len(calls) == 2 == len(rec.calls)
    opts = _ffi.make_solve_opts(TABLE_FIRST if table else None)
    for slot, (first, n) in enumerate([(0, 2), (2, 1)]):
        blk = slice(first, first + n)
        args = check_call(calls[slot], name, update_want(("ctx", 0, slot), n, 2, 2.5, y0[blk], np.full(n, 2.0), consts[blk], r_des[blk], 0.5, 1e-3,
                                                         0, 1e-2, opts, None if popts is None else popts[blk], (0.5, 0.25, 4, 3, 1e-3), 4,
                                                         records_zero=False))      # (the recorder has written them by now)
        o = 15 if table else 14
        in_place = dict(X=o, U=o + 1, NU=o + 2, tf=o + 3, Ks=o + 4, kkt=o + 7, prop_status=o + 8, y_sim=len(args) - 2, sim_status=len(args) - 1)
        for field, i in in_place.items():
            w = getattr(res, field)
            assert np.shares_memory(args[i], w) and args[i].ctypes.data == w[blk].ctypes.data, field
        mark = np.arange(2 * n).reshape(2, n)
        assert np.array_equal(res.status[:, blk], 100 * (slot + 1) + mark) and np.array_equal(res.iters[:, blk], 1000 * (slot + 1) + mark)
    assert res.status.shape == (2, 3) and res.status.dtype == I32 and res.iters.dtype == I32


# ------------------------------------------------------------------------------------------------ scp_iteration_batch
def scp_want(S, Ks, y0, tf, consts, r_des, prop_flags, kind, vec, Ku, Kus, end_tau, disc_flags, opts, popts, reference):
    ref = [Out(S, 7, K), Out(S, 3, K)] if reference else [None, None]
    return [CTX, S, K, Ks, y0, tf, consts, r_des, prop_flags, kind, vec, Ku, Kus, end_tau, 1e-3, disc_flags, 1e-2, opts] + \
           ([] if popts is None else [popts]) + ref + step_outputs(S) + [Out(S, dtype=I32, zero=True)]


LAWS = {"zero": ((_ffi.CTRL_ZERO, None, 0, None), None, None),
        "constant": ((_ffi.CTRL_CONSTANT, [0.1, 0.2, 0.3], 0, None), np.tile(f64([0.1, 0.2, 0.3]), (3, 1)), None),
        "tangential": ((_ffi.CTRL_TANGENTIAL, np.array([0.5]), 0, None), np.full(3, 0.5), None),
        "sequence": ((_ffi.CTRL_SEQUENCE, np.arange(12.0).reshape(3, 4), 4, 0.75), np.tile(np.arange(12.0).reshape(3, 4), (3, 1, 1)), np.full(3, 0.75)),
        "sequence per satellite": ((_ffi.CTRL_SEQUENCE, np.arange(36.0).reshape(3, 3, 4), 4, [0.5, 0.75, 1.0]), np.arange(36.0).reshape(3, 3, 4),
                                   f64([0.5, 0.75, 1.0]))}


@pytest.mark.parametrize("law", list(LAWS))
def test_scp_iteration_thrust_laws(rec, law):
    y0, consts = update_inputs(3)
    (kind, vec, Ku, end_tau), want_vec, want_tau = LAWS[law]
    res = scp_iteration_batch(y0, 1.5, consts, 2.0, (kind, vec, Ku, end_tau), K)
    args = check_call(rec.calls[0], "mpcx_scp_iteration_batch_ragged",
                      scp_want(3, None, y0, np.full(3, 1.5), consts, np.full(3, 2.0), 0, kind, want_vec, Ku, None, want_tau, 0,
                               _ffi.make_solve_opts(), None, False))
    result_is(res, args, 20)
    assert res.prop_status is args[27] and res.xbar is None and res.ubar is None and len(rec.calls) == 1


@pytest.mark.parametrize("table", [False, True])
def test_scp_iteration_counts_reference_and_table(rec, table):
    y0, consts = update_inputs(3)
    options = TABLE_OPTIONS if table else None
    (kind, vec, Ku, end_tau), want_vec, want_tau = LAWS["sequence"]
    res = scp_iteration_batch(y0, 1.5, consts, 2.0, (kind, vec, Ku, end_tau), K, options, Ks=[5, 4, 3], Kus=np.array([4, 3, 2]),
                              return_reference=True, include_drag=True, include_J2=True, rollout_model=True, linear_vt=True)
    name = "mpcx_scp_iteration_batch_ragged_sat" if table else "mpcx_scp_iteration_batch_ragged"
    args = check_call(rec.calls[0], name,
                      scp_want(3, i32([5, 4, 3]), y0, np.full(3, 1.5), consts, np.full(3, 2.0), 3, kind, want_vec, Ku, i32([4, 3, 2]), want_tau, 3,
                               _ffi.make_solve_opts(TABLE_FIRST if table else None, flags=_ffi.SOLVE_LINEAR_VT), _ffi.make_popts(options, 3), True))
    o = 19 if table else 18
    assert res.xbar is args[o] and res.ubar is args[o + 1]
    result_is(res, args, o + 2)
    scp_iteration_batch(y0, 1.5, consts, 2.0, (kind, vec, Ku, end_tau), K, include_drag=True)      # the reference's rollout: no model
    assert (rec.calls[1][1][8], rec.calls[1][1][15]) == (0, 1)


# ------------------------------------------------------------------------------------------------ propagate_batch
def test_propagate_chooses_its_entry_point(rec):
    y0, consts = update_inputs(3)
    tang = (_ffi.CTRL_TANGENTIAL, np.array([0.5]), 0, None)
    (kind, vec, Ku, end_tau), want_vec, want_tau = LAWS["sequence"]
    outs = lambda n: [Out(3, 7, n), Out(3, dtype=I32, zero=True), Out(3, dtype=I32, zero=True)]
    y, status, nsteps = propagate_batch(y0, 1.5, consts, tang, 6, include_drag=True, include_J2=True, max_step=2e-3, device=1, slot=2)
    args = check_call(rec.calls[0], "mpcx_propagate_batch",
                      [("ctx", 1, 2), 3, 6, y0, np.full(3, 1.5), consts, 3, _ffi.CTRL_TANGENTIAL, np.full(3, 0.5), 0, None, 2e-3] + outs(6))
    assert args[3] is y0 and all(a is b for a, b in zip((y, status, nsteps), args[-3:]))
    propagate_batch(y0, [1.0, 2.0, 3.0], consts, tang, [6, 4, 2], include_J2=True)
    check_call(rec.calls[1], "mpcx_propagate_batch_ragged",
               [CTX, 3, 6, i32([6, 4, 2]), y0, f64([1.0, 2.0, 3.0]), consts, 2, _ffi.CTRL_TANGENTIAL, np.full(3, 0.5), 0, None, None, 1e-3] + outs(6))
    propagate_batch(y0, 1.0, consts, (kind, vec, Ku, end_tau), 6, Kus=[4, 3, 2])
    check_call(rec.calls[2], "mpcx_propagate_batch_ragged",
               [CTX, 3, 6, None, y0, np.ones(3), consts, 0, kind, want_vec, Ku, i32([4, 3, 2]), want_tau, 1e-3] + outs(6))
    got = propagate_batch(y0, 1.0, consts, (_ffi.CTRL_CONSTANT, [0.1, 0.2, 0.3], 0, None), 6, thrust=True)
    args = check_call(rec.calls[3], "mpcx_propagate_thrust_batch_ragged",
                      [CTX, 3, 6, None, y0, np.ones(3), consts, 0, _ffi.CTRL_CONSTANT, LAWS["constant"][1], 0, None, None, 1e-3,
                       Out(3, 7, 6), Out(3, 3, 6), Out(3, dtype=I32, zero=True), Out(3, dtype=I32, zero=True)])
    assert len(got) == 4 and got[0] is args[14] and got[3] is args[15] and got[1] is args[16] and got[2] is args[17]
    propagate_batch(y0, 1.0, consts, (_ffi.CTRL_ZERO, None, 0, None), 6, devices=[2])
    check_call(rec.calls[4], "mpcx_propagate_batch", [("ctx", 2, 0), 3, 6, y0, np.ones(3), consts, 0, _ffi.CTRL_ZERO, None, 0, None, 1e-3] + outs(6))
    assert len(rec.calls) == 5


@pytest.mark.parametrize("thrust", [False, True])
def test_propagate_ragged_on_two_contexts_keeps_the_constellations_row_length(rec, thrust):
    y0, consts = update_inputs(3)
    (kind, vec, Ku, end_tau), want_vec, want_tau = LAWS["sequence per satellite"]
    n_eval = [3, 5, 2]                                   # the second block's longest satellite is shorter than the row
    got = propagate_batch(y0, [1.0, 2.0, 3.0], consts, (kind, vec, Ku, end_tau), n_eval, Kus=[4, 3, 2], thrust=thrust, devices=[0, 0])
    name = "mpcx_propagate_thrust_batch_ragged" if thrust else "mpcx_propagate_batch_ragged"
    calls = rec.named(name)
    assert len(calls) == 2 == len(rec.calls) and len(got) == (4 if thrust else 3)
    assert got[0].shape == (3, 7, 5) and got[1].shape == (3,) and (not thrust or got[3].shape == (3, 3, 5))
    whole = [got[0]] + ([got[3]] if thrust else []) + [got[1], got[2]]
    for slot, (first, n) in enumerate([(0, 2), (2, 1)]):
        blk = slice(first, first + n)
        args = check_call(calls[slot], name,
                          [("ctx", 0, slot), n, 5, i32(n_eval[blk]), y0[blk], f64([1.0, 2.0, 3.0])[blk], consts[blk], 0, kind, want_vec[blk], Ku,
                           i32([4, 3, 2])[blk], want_tau[blk], 1e-3, Out(n, 7, 5)] + ([Out(n, 3, 5)] if thrust else [])
                          + [Out(n, dtype=I32, zero=True), Out(n, dtype=I32, zero=True)])
        for a, w in zip(args[14:], whole):
            assert np.shares_memory(a, w) and a.ctypes.data == w[blk].ctypes.data


def test_propagate_uniform_on_two_contexts_is_the_plain_call(rec):
    y0, consts = update_inputs(3)
    y, status, nsteps = propagate_batch(y0, 1.0, consts, (_ffi.CTRL_TANGENTIAL, np.array([0.5]), 0, None), 6, devices=[0, 0])
    calls = rec.named("mpcx_propagate_batch")
    assert len(calls) == 2 == len(rec.calls)
    for slot, (first, n) in enumerate([(0, 2), (2, 1)]):
        blk = slice(first, first + n)
        args = check_call(calls[slot], "mpcx_propagate_batch",
                          [("ctx", 0, slot), n, 6, y0[blk], np.ones(n), consts[blk], 0, _ffi.CTRL_TANGENTIAL, np.full(n, 0.5), 0, None, 1e-3,
                           Out(n, 7, 6), Out(n, dtype=I32, zero=True), Out(n, dtype=I32, zero=True)])
        for a, w in zip(args[12:], (y, status, nsteps)):
            assert np.shares_memory(a, w) and a.ctypes.data == w[blk].ctypes.data


# ------------------------------------------------------------------------------------------------ solve_batch, constraint terms
@pytest.mark.parametrize("table", [False, True])
def test_solve_batch_plain_and_table(rec, table):
    xbar, ubar, consts = step_inputs(3)
    five = [np.arange(3 * (K - 1) * 49.0).reshape(3, K - 1, 7, 7), np.zeros((3, K - 1, 7, 3)), np.ones((3, K - 1, 7, 3)),
            np.zeros((3, 7, K - 1)), np.ones((3, 7, K - 1))]
    options = TABLE_OPTIONS if table else None
    res = solve_batch(*five, xbar, ubar, 1.5, consts, 2.0, options, device=1, fixed_tf=0.5, regularised=True)
    name = "mpcx_solve_batch_sat" if table else "mpcx_solve_batch"
    popts = _ffi.make_popts(options, 3)
    args = check_call(rec.calls[0], name,
                      [("ctx", 1, 0), 3, K] + five + [xbar, ubar, np.full(3, 1.5), consts, np.full(3, 2.0),
                                                       _ffi.make_solve_opts(TABLE_FIRST if table else None, flags=_ffi.SOLVE_FIXED_TF)]
                      + ([] if popts is None else [popts]) + step_outputs(3, tf=np.full(3, 0.5)))
    o = 15 if table else 14
    assert all(a is b for a, b in zip(args[3:10], five + [xbar, ubar]))
    assert res.X is args[o] and res.g_tf is args[o + 3] and np.array_equal(res.tf, np.full(3, 0.5)) and res.tf is not res.g_tf
    check_call(rec.calls[1], "mpcx_solve_regularised", [("ctx", 1, 0), 3, Out(3, 2, dtype=I32, zero=True)])
    assert len(rec.calls) == 2
    with pytest.raises(ValueError):
        solve_batch(*five, xbar, ubar, 1.5, consts, 2.0, TABLE_OPTIONS, shared_tf=True)
    assert len(rec.calls) == 2


@pytest.mark.parametrize("table", [False, True])
def test_constraint_terms_plain_and_table(rec, table):
    xbar, _, consts = step_inputs(3)
    options = TABLE_OPTIONS if table else {"eps_r": 0.02}
    aT, bT, sc = constraint_terms_batch(xbar, consts, [1.0, 2.0, 3.0], options, device=1, linear_vt=True)
    name = "mpcx_constraint_terms_sat" if table else "mpcx_constraint_terms"
    popts = _ffi.make_popts(options, 3)
    args = check_call(rec.calls[0], name,
                      [("ctx", 1, 0), 3, K, xbar, consts, f64([1.0, 2.0, 3.0]),
                       _ffi.make_solve_opts(TABLE_FIRST if table else options, flags=_ffi.SOLVE_LINEAR_VT)]
                      + ([] if popts is None else [popts]) + [Out(3, 8, 7), Out(3, 8), Out(3, _ffi.NTERM_SCALARS)])
    assert aT is args[-3] and bT is args[-2] and sc is args[-1] and len(rec.calls) == 1
