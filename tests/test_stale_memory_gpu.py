"""Solves must not depend on memory they do not own.

Every solver kernel works in memory it did not initialise: the caller's workspace of the _dev entry points (include/mpcx.h
promises nothing about its contents), a workspace slot that persistent workgroups hand from one satellite to the next, the
compute unit's LDS as the previous kernel left it, and -- in ragged launches -- the columns of a row behind a satellite's own
count.  The kernels rely on select masks (`z ? 0.0 : dv`, `dyn`, `act`) and on write-before-read order to make all of that
harmless.  These tests fix the contents of all such memory adversarially and hold ONE property throughout:

    a satellite's results (X, U, NU, tf, kkt, status, iters and the regularisation record) are bit for bit those of the
    same call made with an all-zero workspace, zeroed padding and no history.

The unpoisoned call is pinned to the oracle and the scipy fixtures by the rest of the suite; one poisoned run of a golden
fixture is compared with the oracle directly (test_poisoned_solve_vs_oracle).

Kernels (the dispatcher of solve_api.hip, selected by batch size and flags): one-wave (flags 16), two-wave (flags 32,
S <= 1024), LDS-resident (default, S <= 256, K <= 30), time-parallel (flags 64, S <= 128, row length >= 24), shared-tf (flags 8).
Combinations left out: the shared-tf kernel's ragged cases (it takes no ragged batches: MPCX_E_BADARG) -- the ragged problem set
of section 1 and all of sections 2 and 3 for that kernel.  The time-parallel kernel's K = 4 case is a ragged batch with rows of
length 30 (its K >= 24 rule is on the row length).  Everything else of sections 1-3 runs.

Loop bounds and wait flags (read from the code before the first poisoned run): the interior-point loop's state is in LDS
(SatData::dv, set before the loop), node counts come from the launch arguments, the work-queue counter and the shared-tf
kernel's arrival counter / reduction slots are context-owned and zeroed per launch by the host, and the time-parallel kernel's
mailbox -- the only wait flags inside the caller's workspace -- is zeroed by the host before the launch; every wait has a
spin limit.  No loop bound or wait condition is read from memory these tests fill."""
import numpy as np
import pytest

import dev_solve as D
from test_full_size_gpu import workload
from test_factor_loop_edges_gpu import OPTIMAL_CONTROLLER, THRUST_LIMITED

pytestmark = pytest.mark.gpu

ONE_WAVE, NO_LDS, TIME_PARALLEL, SHARED_TF, LINEAR_VT, INDEX_ORDER = 16, 32, 64, 8, 2, 1
KERNELS = {"one_wave": ONE_WAVE, "two_wave": NO_LDS, "lds": 0, "tp": TIME_PARALLEL, "shared": SHARED_TF}
RAGGED_KERNELS = ("one_wave", "two_wave", "lds", "tp")
PROBLEMS = ("bench_K30", "bench_K4", "optimal_controller_K30", "thrust_limited_K30", "linear_vt_K30", "ragged_K30")
FILLS = ("leftover", "big", "inf", "nan-", "nan+")       # in this order: the workspace of another solve, +-1e300, +Inf, quiet NaN
S_SMALL = 32
CASES = [(k, p) for k in KERNELS for p in PROBLEMS if not (k == "shared" and p == "ragged_K30")]
assert len(CASES) == len(KERNELS) * len(PROBLEMS) - 1

_cache = {}


def cached_workload(K, first, count):
    key = (K, first, count)
    if key not in _cache:
        _cache[key] = workload(4096, K, first=first, count=count)
    return tuple(a.copy() for a in _cache[key])


def truncated(S, Ks, first=0):
    """ragged batch: the first Ks[s] nodes of a 30-node rollout over tf = 1, flown in tf = (Ks - 1) / 29 -- a consistent
    reference on the grid linspace(0, 1, Ks[s]); zeroed padding"""
    x, u, c, _ = cached_workload(30, first, S)
    Ks = np.asarray(Ks, dtype=np.int32)
    for s in range(S):
        x[s, :, Ks[s]:] = 0.0; u[s, :, Ks[s]:] = 0.0
    r_des = np.array([np.linalg.norm(x[s, :3, Ks[s] - 1]) for s in range(S)])
    return dict(x=x, u=u, tf=(Ks - 1) / 29.0, c=c, rd=r_des, Ks=Ks)


def problem(name, kernel, S=S_SMALL):
    """-> dict(x, u, tf, c, rd, Ks, options, flags)"""
    if name == "ragged_K30":
        p = truncated(S, 3 + (np.arange(S) * 11) % 28)
        assert p["Ks"].min() == 3 and p["Ks"].max() == 30
    elif name == "bench_K4" and kernel == "tp":
        # the time-parallel kernel is chosen by the row length: rows of 30 columns, four nodes in use (one segment)
        x4, u4, c, rd = cached_workload(4, 0, S)
        x = np.zeros((S, 7, 30)); u = np.zeros((S, 3, 30)); x[:, :, :4] = x4; u[:, :, :4] = u4
        p = dict(x=x, u=u, tf=np.ones(S), c=c, rd=rd, Ks=np.full(S, 4, dtype=np.int32))
    else:
        K = 4 if name == "bench_K4" else 30
        x, u, c, rd = cached_workload(K, 0, S)
        p = dict(x=x, u=u, tf=np.ones(S), c=c, rd=rd, Ks=None)
    p["options"] = {"optimal_controller_K30": OPTIMAL_CONTROLLER, "thrust_limited_K30": THRUST_LIMITED}.get(name, {})
    p["flags"] = KERNELS[kernel] | (LINEAR_VT if name == "linear_vt_K30" else 0)
    return p


def other_problem(kernel, S=S_SMALL):
    """what leaves the workspace behind for fill 'leftover': other satellites, 30 nodes, the linearised tangential pair
    (G_SVT / G_ZVT in use) and a thrust limit below the reference thrust, on the same kernel"""
    x, u, c, rd = cached_workload(30, 1000, S)
    return dict(x=x, u=u, tf=np.ones(S), c=c, rd=rd, Ks=None, options=THRUST_LIMITED, flags=KERNELS[kernel] | LINEAR_VT)


def assert_kernel(kernel, S, K, flags):
    """the call takes the intended kernel: the dispatcher's own conditions (solve_api.hip: choose_kernel), by batch size, row length, flags"""
    tp = bool(flags & TIME_PARALLEL) and S <= 128 and K >= 24
    if kernel == "shared":
        assert flags & SHARED_TF
        return
    assert not flags & SHARED_TF
    if kernel == "tp":
        assert tp
    elif kernel == "lds":
        assert not tp and S <= D.n_slots() // 8 and K <= 30 and not flags & (ONE_WAVE | NO_LDS)
    elif kernel == "two_wave":
        assert not tp and S <= 1024 and flags & NO_LDS and not flags & ONE_WAVE
    else:
        assert not tp and flags & ONE_WAVE


def slot_stride(kernel, K):
    return D.ws_doubles_tp(K) if kernel == "tp" else D.ws_doubles(K)


def stages_of(p, disc_flags=0):
    """stage records of a problem (zero behind a satellite's last interval)"""
    import torch
    x = D.dev(p["x"])
    S, _, K = x.shape
    stage = torch.zeros((S, K - 1, D.STAGE_DOUBLES), dtype=torch.float64, device=x.device)
    stage, st = D.discretize_stages(p["x"], p["u"], p["tf"], p["c"], Ks=p["Ks"], Kus=p["Ks"], flags=disc_flags, stage=stage)
    assert (st == 0).all()
    return stage


def run(mode, p, ws=None, stage=None):
    opts = D.make_opts(p["options"], flags=p["flags"])
    if mode == "solve":
        return D.solve_dev(stage, p["x"], p["u"], p["tf"], p["c"], p["rd"], opts, Ks=p["Ks"], ws=ws)
    return D.step_dev(p["x"], p["u"], p["tf"], p["c"], p["rd"], opts, Ks=p["Ks"], ws=ws)


def assert_same(base, got, what, rows=None):
    for f in D.FIELDS:
        a, b = base[f], got[f]
        if rows is not None:
            a = a[rows]
        assert D.same_bits(a, b), (what, f, int(np.sum(np.ascontiguousarray(a) != np.ascontiguousarray(b))))


def assert_defined(r, Ks, K, what):
    """section 5: the result tensors went in holding NaN / -1; everything the header promises is defined afterwards"""
    S = len(r["status"])
    Ks = np.full(S, K) if Ks is None else Ks
    assert (r["status"] >= 0).all() and (r["iters"] >= 0).all() and (r["n_regularised"] >= 0).all(), what
    assert ((r["first_regularised"] == -1) == (r["n_regularised"] == 0)).all() and (r["first_regularised"] >= -1).all(), what
    assert not np.isnan(r["tf"]).any() and not np.isnan(r["kkt"][r["status"] != 6]).any(), what
    for s in range(S):
        k = Ks[s]
        if r["status"][s] in (0, 5, 7):
            assert np.isfinite(r["X"][s][:, :k]).all() and np.isfinite(r["U"][s][:, :k]).all() and np.isfinite(r["NU"][s][:, :k]).all(), (what, s)
        if r["status"][s] not in (8, 9):            # (rejected satellites get their reference rows back whole: include/mpcx.h)
            assert not r["X"][s][:, k:].any() and not r["U"][s][:, k:].any() and not r["NU"][s][:, k:].any(), (what, s)
        assert not np.isnan(r["NU"][s][:, k - 1]).any()


# ---- 1. workspace contents ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel,name", CASES)
def test_workspace_contents_do_not_matter(kernel, name):
    import torch
    p = problem(name, kernel)
    S, _, K = p["x"].shape
    D.check_layout(K)
    assert_kernel(kernel, S, K, p["flags"])
    q = other_problem(kernel)
    assert_kernel(kernel, S, 30, q["flags"])
    stride = slot_stride(kernel, K)
    for mode in ("solve", "step"):
        stage = stages_of(p) if mode == "solve" else None
        n = max(D.solver_workspace_doubles(S, K), D.solver_workspace_doubles(S, 30))
        off = 0
        if mode == "step":
            off = D.step_header_doubles(S, K)
            n = max(off + D.solver_workspace_doubles(S, K), D.step_workspace_doubles(S, 30))
        base, _, _ = run(mode, p, D.filled(n, "zero"), stage)
        assert_defined(base, p["Ks"], K, (kernel, name, mode))
        assert (base["iters"] > 0).all() and not np.isin(base["status"], (8, 9, 10)).any(), (kernel, name, mode, base["status"])
        for fill in FILLS:
            what = (kernel, name, mode, fill)
            if fill == "leftover":
                ws = D.filled(n, "zero")
                left, ws, _ = run(mode, q, ws, stages_of(q) if mode == "solve" else None)
                assert (left["iters"] > 0).all(), what
            else:
                ws = D.filled(n, fill)
                assert {"big": lambda t: (t.abs() == 1e300).all() and (t[0] > 0) and (t[1] < 0), "inf": lambda t: torch.isinf(t).all(),
                        "nan-": lambda t: torch.isnan(t).all() and (D.bits(t) < 0).all(),
                        "nan+": lambda t: torch.isnan(t).all() and (D.bits(t) > 0).all()}[fill](ws), what
            ptr = ws.data_ptr()
            snap = D.bits(ws).clone()
            slots_before = snap[off:off + S * stride].view(S, stride)
            if fill == "leftover":
                # (the other solve's slots are those of 30 nodes: a shorter test's slot may fall into a stretch it never wrote -- the
                #  LDS-resident kernel keeps most of its working set out of the workspace -- so the leftovers are held to be there as a whole)
                assert (slots_before != 0).any(), what
            else:
                assert (slots_before != 0).all(), what                          # every double of every slot in use holds the fill
            got, ws_after, _ = run(mode, p, ws, stage)
            assert ws_after is ws and ws.data_ptr() == ptr, what                # the tensor that was filled is the one that was passed
            slots_after = D.bits(ws)[off:off + S * stride].view(S, stride)
            assert (slots_after != slots_before).any(dim=1).all(), what         # ... and every slot in use was worked in
            if mode == "step":
                assert (D.bits(ws)[:off] != snap[:off]).any(), what             # (stage records and discretize status)
            if kernel == "tp":
                assert (got["status"] != 10).all(), what                        # the time-parallel kernel ran to its end
            assert_same(base, got, what)


# ---- the one direct anchor: a poisoned run against the oracle ---------------------------------------------------------------

def test_poisoned_solve_vs_oracle(golden_dir):
    """golden fixture tan_K30_tf1 through the device-pointer solve in a workspace of 0xFF bytes, against oracle/nlp_ipm.py under
    test_solve_vs_oracle's own rule (test_solve_gpu.solution_tolerance)"""
    import torch
    from test_solve_gpu import load, oracle_solve, solution_tolerance
    d, x, u, tf, cst = load(golden_dir, "tan_K30_tf1")
    K = x.shape[1]
    r_des = float(np.linalg.norm(x[:3, -1]))
    _, ref = oracle_solve(x, u, tf, cst, r_des, {k: d[k] for k in ("A", "Bp", "Bn", "Sigma", "xi")})
    # packed stage records [A | B_kn | B_kp | Sigma | xi] (include/mpcx.h, MPCX_STAGE_DOUBLES)
    stage = np.concatenate([d["A"].reshape(K - 1, 49), d["Bn"].reshape(K - 1, 21), d["Bp"].reshape(K - 1, 21), d["Sigma"].T, d["xi"].T], axis=1)
    assert stage.shape == (K - 1, D.STAGE_DOUBLES)
    ws = D.filled(D.solver_workspace_doubles(1, K), "nan-")
    assert torch.isnan(ws).all()
    res, _, _ = D.solve_dev(stage[None], x[None], u[None], [tf], cst[None], [r_des], D.make_opts({}), ws=ws)
    assert not torch.isnan(ws[:D.ws_doubles(K)]).all()
    assert ref["status"] == 0 and res["status"][0] == 0 and res["kkt"][0] <= 1e-8
    tol = solution_tolerance(ref, res["iters"][0], int(res["n_regularised"][0]), int(res["first_regularised"][0]))
    assert np.abs(res["X"][0] - ref["X"]).max() < tol and np.abs(res["U"][0] - ref["U"]).max() < tol
    assert np.abs(res["NU"][0] - ref["NU"]).max() < tol and abs(res["tf"][0] - ref["tf"]) < tol


# ---- 2. slot reuse ----------------------------------------------------------------------------------------------------------

def test_second_occupant_of_a_slot_sees_nothing_of_the_first():
    """One-wave kernel, more satellites than workspace slots: the 256 satellites that take a slot second have 3..29 nodes and
    find, behind their own last node, the records of a 30-node predecessor.  Every one of them, and a sample of the first
    occupants, against the same satellite solved in a batch that holds no more satellites than slots."""
    slots = D.n_slots()
    n_tail = 256
    S = slots + n_tail
    Ks = np.full(S, 30, dtype=np.int32)
    Ks[slots:] = 3 + (np.arange(n_tail) * 7) % 27
    assert S > slots and Ks[slots:].max() < 30 and Ks[slots:].min() == 3 and (Ks[:slots] == 30).all()
    p = truncated(S, Ks)
    p["options"] = THRUST_LIMITED
    sample = np.concatenate([np.arange(0, slots, 32), np.arange(slots, S)])
    sub = {k: (v[sample].copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()}
    assert len(sample) <= slots
    sub["flags"] = ONE_WAVE | INDEX_ORDER
    base, _, _ = run("step", sub)
    assert (base["iters"] > 0).all() and not np.isin(base["status"], (8, 9)).any()
    assert_defined(base, sub["Ks"], 30, "tail batch")
    # index order: workgroup b starts with satellite b, the tail follows into the slots that come free
    p["flags"] = ONE_WAVE | INDEX_ORDER
    got, ws, _ = run("step", p)
    assert_same(got, base, "index order", rows=sample)
    # longest first: the default order, from the second call of the same size on (the predictor then has a solve to go by);
    # both calls in the workspace the index-order call left behind
    p["flags"] = ONE_WAVE
    for call in (1, 2):
        got, ws, _ = run("step", p, ws)
        assert_same(got, base, ("longest first", call), rows=sample)
    # the batch reversed: the short satellites take the slots first, the long ones second
    rev = {k: (v[::-1].copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()}
    rev["flags"] = ONE_WAVE | INDEX_ORDER
    got, ws, _ = run("step", rev, ws)
    assert_same({f: got[f][::-1] for f in D.FIELDS}, base, "reversed", rows=sample)


# ---- 3. padding ---------------------------------------------------------------------------------------------------------------

def poison_padding(p, value):
    import torch
    x, u = D.dev(p["x"]).clone(), D.dev(p["u"]).clone()
    S, _, K = x.shape
    pad = torch.arange(K, device=x.device)[None, :] >= D.dev(p["Ks"])[:, None].to(torch.int64)       # [S][K]: columns behind the count
    x[pad[:, None, :].expand(S, 7, K)] = value
    u[pad[:, None, :].expand(S, 3, K)] = value
    return x, u, pad


@pytest.mark.parametrize("kernel", RAGGED_KERNELS)
def test_padding_contents_do_not_matter(kernel):
    """ragged solve and ragged fused step: the columns Ks[s]..K-1 of xbar and ubar (in the fused step ubar is the thrust table,
    Kus = Ks) and the stage records behind interval Ks[s]-2 hold NaN, then 1e300"""
    import torch
    p = problem("ragged_K30", kernel)
    S, _, K = p["x"].shape
    assert_kernel(kernel, S, K, p["flags"])
    assert (p["Ks"] < 24).any() and (p["Ks"] < K).sum() >= S - 2        # (the time-parallel batch holds short satellites too)
    stage0 = stages_of(p)
    for mode in ("solve", "step"):
        base, _, _ = run(mode, p, None, stage0)
        assert (base["iters"] > 0).all() and not np.isin(base["status"], (8, 9, 10)).any()
        for value in (float("nan"), 1e300):
            x, u, pad = poison_padding(p, value)
            stage = stage0.clone()
            stage[pad[:, 1:, None].expand(S, K - 1, D.STAGE_DOUBLES)] = value      # record k belongs to satellite s while k + 1 < Ks[s]
            held = (lambda t: torch.isnan(t).all()) if value != value else (lambda t: (t == value).all())
            assert held(x[pad[:, None, :].expand(S, 7, K)]) and held(u[pad[:, None, :].expand(S, 3, K)]) and pad.sum() > 0
            assert held(stage[pad[:, 1:]]) and torch.isfinite(stage[~pad[:, 1:]]).all()
            q = dict(p, x=x, u=u)
            got, _, _ = run(mode, q, None, stage)
            if kernel == "tp":
                assert (got["status"] != 10).all()
            assert_same(base, got, (kernel, mode, value))
            assert_defined(got, p["Ks"], K, (kernel, mode, value))


def test_padding_of_the_ragged_discretisation():
    """mpcx_discretize_stages_ragged_dev with NaN / 1e300 behind every satellite's columns: the records in use are bit for bit
    those of the rectangular single-satellite call"""
    import torch
    p = problem("ragged_K30", "one_wave")
    S, _, K = p["x"].shape
    for value in (float("nan"), 1e300):
        x, u, pad = poison_padding(p, value)
        assert pad.sum() > 0 and (torch.isnan(x[pad[:, None, :].expand(S, 7, K)]).all() if value != value else (x[pad[:, None, :].expand(S, 7, K)] == value).all())
        stage, st = D.discretize_stages(x, u, p["tf"], p["c"], Ks=p["Ks"], Kus=p["Ks"])
        assert (st == 0).all()
        stage = stage.cpu().numpy()
        for s in range(0, S, 3):
            k = int(p["Ks"][s])
            one, st1 = D.discretize_stages(p["x"][s:s + 1, :, :k].copy(), p["u"][s:s + 1, :, :k].copy(), p["tf"][s:s + 1], p["c"][s:s + 1])
            assert st1[0] == 0 and D.same_bits(stage[s, :k - 1], one.cpu().numpy()[0]), (value, s, k)


def test_padding_of_the_ragged_sequence_rollout():
    """mpcx_propagate_thrust_batch_ragged_dev playing SEQUENCE tables of Kus[s] columns with NaN / 1e300 behind them, sampled at
    n_evals[s] points: every satellite against its own rectangular call; the _dev call leaves the output columns behind a
    satellite's count as they were (include/mpcx.h)"""
    S = 16
    p = truncated(S, 2 + (np.arange(S) * 7) % 29)
    Kus = p["Ks"]
    assert Kus.min() == 2 and Kus.max() == 30
    n_evals = (1 + (np.arange(S) * 11) % 40).astype(np.int32); n_eval = 40
    end_tau = np.where(np.arange(S) % 3 == 0, 0.7, 1.0)
    y0 = p["x"][:, :, 0].copy()
    tf = np.full(S, 0.5)
    for value in (float("nan"), 1e300):
        _, table, pad = poison_padding(p, value)
        assert pad.sum() > 0
        y, uo, st, ns = D.propagate_thrust_dev(y0, tf, p["c"], table, end_tau, n_eval, n_evals=n_evals, Kus=Kus)
        assert (st == 0).all()
        for s in range(S):
            k, n = int(Kus[s]), int(n_evals[s])
            y1, u1, st1, ns1 = D.propagate_thrust_dev(y0[s:s + 1], tf[s:s + 1], p["c"][s:s + 1], p["u"][s:s + 1, :, :k].copy(), end_tau[s:s + 1], n)
            assert st1[0] == 0 and ns1[0] == ns[s]
            assert D.same_bits(y[s][:, :n], y1[0]) and D.same_bits(uo[s][:, :n], u1[0]), (value, s)
            assert np.isnan(y[s][:, n:]).all() and np.isnan(uo[s][:, n:]).all()


# ---- 4. call history on one context, host-pointer API ------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", ["lds", "tp"])
def test_call_history_of_a_context_does_not_matter(kernel):
    """mpc_step_batch of problem B after a larger, different problem A on the same context (the context's arena, its workspace
    and the LDS of the compute units hold A's leftovers), after B itself, and on a context created for it: one set of bits.
    On the two kernels whose LDS working set cannot be filled from outside."""
    from mpconstellation_amd import mpc_step_batch
    flags = KERNELS[kernel]
    xa, ua, ca, ra = cached_workload(30, 500, 96)
    xb, ub, cb, rb = cached_workload(24, 0, 32)
    assert_kernel(kernel, 96, 30, flags | LINEAR_VT); assert_kernel(kernel, 32, 24, flags)
    used, fresh = (41, 42) if kernel == "lds" else (43, 44)            # context slots no other test takes
    A = lambda slot: mpc_step_batch(xa, ua, np.ones(96), ca, ra, options=THRUST_LIMITED, flags=flags | LINEAR_VT, slot=slot, regularised=True)
    B = lambda slot: mpc_step_batch(xb, ub, np.ones(32), cb, rb, flags=flags, slot=slot, regularised=True)
    a = A(used)
    assert (a.iters > 0).all()
    after_a, after_b, alone = B(used), B(used), B(fresh)
    assert np.isin(alone.status, (0, 7)).all()
    for r, what in ((after_a, "after A"), (after_b, "after B")):
        if kernel == "tp":
            assert (r.status != 10).all()
        for f in D.FIELDS:
            assert D.same_bits(getattr(alone, f), getattr(r, f)), (kernel, what, f)


# ---- 5. output buffers --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", list(KERNELS))
def test_every_promised_output_is_written(kernel):
    """Result tensors go in holding NaN (status, iters, the regularisation record: -1).  include/mpcx.h: the _dev solves write
    every element of a satellite's rows -- zeros behind its count; a satellite that comes back MPCX_ST_BADK or
    MPCX_ST_INFEASIBLE gets its reference rows back whole, padding included."""
    ragged = kernel != "shared"
    p = problem("ragged_K30" if ragged else "bench_K30", kernel)
    S, _, K = p["x"].shape
    if ragged:
        x, u, pad = poison_padding(p, 1e300)
        p = dict(p, x=x, u=u)
        Ks = p["Ks"].copy(); Ks[5] = 2; Ks[9] = K + 1            # two counts the solver cannot take
        rd = p["rd"].copy(); rd[7] = 7.0                          # one target outside r_max: an empty constraint set
        p = dict(p, Ks=Ks, rd=rd)
    for mode in ("solve", "step"):
        got, _, _ = run(mode, p, None, stages_of(problem("ragged_K30" if ragged else "bench_K30", kernel)) if mode == "solve" else None)
        assert_defined(got, p["Ks"].clip(3, K) if ragged else None, K, (kernel, mode))
        if ragged:
            assert got["status"][5] == 9 and got["status"][9] == 9 and got["status"][7] == 8
            xin, uin = p["x"].cpu().numpy(), p["u"].cpu().numpy()
            for s in (5, 7, 9):
                assert D.same_bits(got["X"][s], xin[s]) and D.same_bits(got["U"][s], uin[s]) and not got["NU"][s].any()
                assert got["iters"][s] == 0 and got["n_regularised"][s] == 0 and got["first_regularised"][s] == -1
            assert not np.isin(np.delete(got["status"], (5, 7, 9)), (8, 9, 10)).any()
