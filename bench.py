#!/usr/bin/env python3
"""bench.py -- satellite-MPC-steps/s of the fused discretize+solve hot path on MI355X.

One "step" = one pass of the hot path (Discretizer.discretize + get_constraint_terms + solve_OPT of
the reference, one SCP iteration) over every satellite of the batch, inputs resident in HBM.
Prints ONE JSON line (rank 0).  See DESIGN.md "Measurement".  A plain run measures the headline only (set-up, warm-up,
the timed steps, the line); --full adds the secondary measurements, --dump-outputs DIR writes the last step's results.

`python bench.py --gpus N` starts N ranks itself (torch.distributed.run, one process per GPU, before this process has
touched a GPU); under an outer launcher (WORLD_SIZE set) it is one of the ranks."""
import argparse
import ctypes as C
import glob
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

WORKLOADS = {            # BASELINE.json configs: name -> (satellites per GPU, nodes K, SCP iterations per MPC step)
    "S64_K30": (64, 30, 1),            # configs[1]
    "S4096_K30": (4096, 30, 1),        # configs[2]: the N = 30 single-GPU configuration the target is stated for
    "S4096_K100_scp2": (4096, 100, 2), # configs[3]: 2 SCP iterations with nonlinear re-rollout (control.py:166,183-227)
    "S8192_K30": (8192, 30, 1),        # configs[4] per GPU (65,536 over 8)
}
DEFAULT_SINGLE = "S4096_K30"      # the same per-GPU work at every N (weak scaling); configs[4]'s 8192 per GPU rides along as `also` when N > 1 (--full)
F64_VALU_PEAK_TFLOPS = 78.6     # MI355X fp64 vector peak
FLOP_PER_NODE_ITER = 18e3       # factorisation 8.7k + 8-channel sweeps 7k + node-parallel phases 2.4k
HBM_PEAK_GBPS = 8000.0   # MI355X_MICROARCH.md chip table


def algorithmic_bytes(K):
    """compulsory traffic of one satellite-MPC-step (one SCP iteration): read xbar(7K) ubar(3K) tf
    consts(5), write x(7K) u(3K) nu(7K) tf status = 8(27K+7)+8 bytes, plus -- discretize and solve being two kernels --
    the stage records A, B+-, Sigma, xi written by one and read by the other: 2 x 840 (K-1) bytes."""
    return 8 * (27 * K + 7) + 8 + 1680 * (K - 1)


N_VARIANTS = 4           # consecutive steps solve similar, not identical, problems (see Runner)
REF_THRUST = (0.50, 0.51, 0.49, 0.505)


class Runner:
    """Device-resident state of one workload on one GPU; step() enqueues one MPC step for every satellite.
    Consecutive steps cycle through N_VARIANTS reference trajectories of the same constellation (tangential reference
    thrust 0.50 / 0.51 / 0.49 / 0.505): like the steps of a closed MPC loop they pose similar but not identical problems,
    so the solver's longest-first launch order (sorted by the PREVIOUS solve's iteration counts) is the imperfect
    predictor it is in use, not the exact one identical inputs would make it."""

    def __init__(self, workload, rank, world, local_rank, n_variants=N_VARIANTS):
        import torch
        from mpconstellation_amd import _ffi
        from mpconstellation_amd.constellation import constellation_states, normalize_batch, tangential_thrust
        from mpconstellation_amd.simulator import propagate_batch
        from mpconstellation_amd.sharding import shard_block
        self.torch, self.ffi = torch, _ffi
        self.lib = _ffi.load(); self.ctx = _ffi.context(local_rank)
        self.stream = torch.cuda.current_stream().cuda_stream
        S, K, n_scp = WORKLOADS[workload]
        self.S, self.K, self.n_scp = S, K, n_scp
        S_total = S * world
        first, count = shard_block(S_total, world, rank)        # contiguous block, no exchange
        assert count == S
        states = constellation_states(S_total, first=first, count=S)
        y0, consts = normalize_batch(states)
        tfbar = np.ones(S)
        dev = torch.device("cuda", local_rank)
        t64 = dict(dtype=torch.float64, device=dev)
        T = lambda a: torch.tensor(a, **t64)
        self.variants = []
        for mag in REF_THRUST[:n_variants]:
            xbar, st, _ = propagate_batch(y0, tfbar, consts, (_ffi.CTRL_TANGENTIAL, np.array([mag]), 0, None), K, device=local_rank)
            assert (st == 0).all()
            ubar = np.ascontiguousarray(tangential_thrust(xbar, mag))
            r_des = np.linalg.norm(xbar[:, 0:3, -1], axis=1)
            self.variants.append(dict(host=dict(xbar=xbar, ubar=ubar, tfbar=tfbar, consts=consts, r_des=r_des),
                                      d_x0=T(xbar), d_u0=T(ubar), d_rd=T(r_des)))
        self.n_steps = 0
        self.host = self.variants[0]["host"]
        self.d_tf0 = T(tfbar)
        self.d_x0, self.d_u0, self.d_rd = (self.variants[0][k] for k in ("d_x0", "d_u0", "d_rd"))
        self.d_x, self.d_u, self.d_tf = self.d_x0.clone(), self.d_u0.clone(), self.d_tf0.clone()
        self.d_c, self.d_y0, self.d_one = T(consts), T(y0), T(np.ones(S))
        self.d_X = torch.empty((S, 7, K), **t64); self.d_U = torch.empty((S, 3, K), **t64); self.d_NU = torch.empty((S, 7, K), **t64)
        self.d_tfo = torch.empty(S, **t64); self.d_kkt = torch.empty(S, **t64)
        i32 = dict(dtype=torch.int32, device=dev)
        self.d_st = torch.empty(S, **i32); self.d_it = torch.empty(S, **i32); self.d_dst = torch.empty(S, **i32)
        self.d_pst = torch.empty(S, **i32); self.d_pns = torch.empty(S, **i32); self.d_rst = torch.empty(S, **i32)
        self.base_res = K          # tf_bar = 1: K = int(base_res * tf) nodes (simulator.py:38)
        self.d_Kn = [torch.empty(S, **i32) for _ in range(2)]        # node counts of the SCP iterations (alternating: the buffer
        self.d_Knf = torch.empty(S, **t64)                           # an iteration reads stays untouched while the next is written)
        self.d_stage = torch.empty((S, K - 1, _ffi.STAGE_DOUBLES), **t64)
        self.d_ws = torch.empty(self.lib.mpcx_solve_workspace_bytes(S, K) // 8 + 8, **t64)
        self.opts = _ffi.make_solve_opts({})
        self.stream = torch.cuda.current_stream().cuda_stream
        self.solve_events = []
        self.first_status = None     # per SCP iteration: status / iterations of the last step (SCP workloads)

    def step(self, record=False):
        torch, lib, ctx, ffi = self.torch, self.lib, self.ctx, self.ffi
        p = lambda t: C.c_void_p(t.data_ptr())
        S, K = self.S, self.K
        st = C.c_void_p(self.stream)
        v = self.variants[self.n_steps % len(self.variants)]; self.n_steps += 1
        self.host = v["host"]; self.d_x0, self.d_u0, self.d_rd = v["d_x0"], v["d_u0"], v["d_rd"]
        if self.n_scp > 1:                      # every MPC step starts from its variant's reference rollout
            self.d_x.copy_(self.d_x0); self.d_u.copy_(self.d_u0); self.d_tf.copy_(self.d_tf0)
        else:
            self.d_x, self.d_u = self.d_x0, self.d_u0                            # (pointers only: inputs stay resident)
        ks = None                               # node counts of this SCP iteration (None: K for every satellite)
        for it in range(self.n_scp):
            # the two launches of mpcx_mpc_step_batch[_ragged]_dev, issued separately so the solve can be bracketed by events
            ffi.check(lib.mpcx_discretize_stages_ragged_dev(ctx, S, K, ks, K, ks, p(self.d_x), p(self.d_u), p(self.d_tf), p(self.d_c), 0,
                                                            1e-2, p(self.d_stage), p(self.d_dst), st), ctx, "discretize")
            if record:
                e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True); e0.record()
            ffi.check(lib.mpcx_solve_batch_ragged_dev(ctx, S, K, ks, p(self.d_stage), p(self.d_x), p(self.d_u), p(self.d_tf), p(self.d_c),
                                                      p(self.d_rd), C.byref(self.opts), p(self.d_X), p(self.d_U), p(self.d_NU), p(self.d_tfo),
                                                      p(self.d_st), p(self.d_it), p(self.d_kkt), p(self.d_ws), st), ctx, "solve")
            if record:
                e1.record(); self.solve_events.append((e0, e1))
            if self.n_scp > 1 and it + 1 < self.n_scp:
                # SCP re-linearisation point (control.py:221,227): nonlinear rollout under the optimised FOH sequence over
                # tf_u, sampled -- as the reference does, simulator.py:38 -- at int(base_res * tf_u) nodes, a different
                # count for every satellite: the next iteration is a ragged launch (rows of length K, Kn[s] columns in
                # use).  The new reference thrust is extract_uk of that sequence at the rollout's nodes.
                kn = self.d_Kn[it % 2]
                torch.mul(self.d_tfo, float(self.base_res), out=self.d_Knf); kn.copy_(self.d_Knf)      # int(base_res * tf_u): copy_ truncates
                ffi.check(lib.mpcx_propagate_batch_ragged_dev(ctx, S, K, p(kn), p(self.d_y0), p(self.d_tfo), p(self.d_c), 0,
                                                              ffi.CTRL_SEQUENCE, p(self.d_U), K, ks, p(self.d_one), 1e-3, p(self.d_x),
                                                              p(self.d_pst), p(self.d_pns), st), ctx, "propagate")
                ffi.check(lib.mpcx_resample_sequence_dev(ctx, S, K, ks, p(self.d_U), K, p(kn), p(self.d_u), p(self.d_rst), st),
                          ctx, "resample")
                self.d_tf.copy_(self.d_tfo)
                ks = p(kn)

    def solver_stats(self):
        status = self.d_st.cpu().numpy(); dstat = self.d_dst.cpu().numpy()
        status = np.where(dstat != 0, dstat, status)
        return status, self.d_it.cpu().numpy(), self.d_kkt.cpu().numpy()


def measure(runner, steps, warmup, world):
    import torch
    import torch.distributed as dist
    for _ in range(warmup):
        runner.step()
    torch.cuda.synchronize()
    if world > 1: dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        runner.step(record=True)
    torch.cuda.synchronize()
    if world > 1: dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if world > 1:
        dev = "cpu" if dist.get_backend() == "gloo" else "cuda"
        tt = torch.tensor([elapsed], dtype=torch.float64, device=dev); dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
    solve_ms = float(np.mean([a.elapsed_time(b) for a, b in runner.solve_events]))
    return elapsed, solve_ms


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(runner, status, iters, kkt, out_dir, rank, world):
    """--dump-outputs: what a caller of the timed path receives from its last step (the last SCP iteration's solve: X, U,
    nu, tf, status with the discretisation's folded in as in solver_stats, iterations, KKT residual) as float64 .npy files,
    one per array (with N > 1 every rank writes its own block, <name>.rank<r>.npy).  Above 64 MB in all, a fixed seeded
    sample of satellites is written instead, and its indices as satellite_index.npy."""
    arrays = {"X": runner.d_X.cpu().numpy(), "U": runner.d_U.cpu().numpy(), "NU": runner.d_NU.cpu().numpy(),
              "tf": runner.d_tfo.cpu().numpy(), "status": status, "iters": iters, "kkt": kkt}
    arrays = {k: np.asarray(v, dtype=np.float64) for k, v in arrays.items()}
    S = runner.S
    per_satellite = sum(a.nbytes for a in arrays.values()) / S
    if per_satellite * S > DUMP_LIMIT_BYTES:
        idx = np.sort(np.random.default_rng(0).choice(S, int(DUMP_LIMIT_BYTES // (per_satellite + 8)), replace=False))
        arrays = {k: v[idx] for k, v in arrays.items()}
        arrays["satellite_index"] = idx.astype(np.float64)
    os.makedirs(out_dir, exist_ok=True)
    suffix = f".rank{rank}" if world > 1 else ""
    for k, v in arrays.items():
        np.save(os.path.join(out_dir, k + suffix + ".npy"), v)


def _committed_counters(fname, workload, kernel):
    """One kernel's entry of the newest committed counter summary profiles/rNN/<fname> that holds the workload -- a counter
    measurement of an earlier run on another box, echoed here; it is reported only when the kernel sources are byte for byte
    the ones that were profiled (the profile records their hashes) and the build flags the same, with its origin."""
    import hashlib
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", fname)), reverse=True):
        prof = json.load(open(f))
        ks = prof.get("workloads", {}).get(workload, {})
        # (batches of up to 1024 run on the two-wave build's kernel, of up to one satellite per compute unit on the LDS-resident one)
        w = ks.get(kernel) or ks.get(kernel + "_lds") or ks.get(kernel + "2w")
        if not w: continue
        src = os.path.relpath(f, ROOT)
        want = prof.get("kernel_source_sha256")
        if not want:
            return None, f"{src}: no source hashes recorded (profile of an earlier round), not reported"
        for name, h in want.items():
            path = os.path.join(ROOT, "mpconstellation_amd", "csrc", name)
            if not os.path.exists(path) or hashlib.sha256(open(path, "rb").read()).hexdigest() != h:
                return None, f"{src}: {name} changed since it was profiled, not reported"
        if prof.get("build_flags"):
            from mpconstellation_amd import build as _b
            if prof["build_flags"] != " ".join(_b.FLAGS):
                return None, f"{src}: build flags changed since it was profiled, not reported"
        return w, f"{src} (same kernel sources, counters of that profiling run)"
    return None, "no committed profile holds this workload"


def measured_traffic(workload, kernel="solve_kernel"):
    """HBM bytes per launch from the committed rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes (profiles/rNN/pmc_traffic.json)"""
    w, src = _committed_counters("pmc_traffic.json", workload, kernel)
    return (w["hbm_bytes_per_launch"] if w else None), src


def measured_fp64_flop(workload, kernel="solve_kernel"):
    """fp64 operations one launch EXECUTES, 64 lanes per wave instruction, from the committed SQ_INSTS_VALU_{FMA,MUL,ADD}_F64
    passes (profiles/rNN/pmc_sq.json: 64 x (2 FMA + MUL + ADD)); idle lanes of a wave instruction count as executed"""
    w, src = _committed_counters("pmc_sq.json", workload, kernel)
    return (w.get("fp64_flop_64lanes") if w else None), src


def roofline(workload, S, K, solve_ms, iters):
    B = algorithmic_bytes(K)
    achieved = S * B / (solve_ms * 1e-3) / 1e9           # dominant kernel: solve_kernel, one launch = S satellites
    useful = FLOP_PER_NODE_ITER * K * float(iters.sum())  # of the last solve_kernel launch on this rank
    traffic, traffic_source = measured_traffic(workload)
    executed, flop_source = measured_fp64_flop(workload)
    tf = lambda fl: None if fl is None else fl / (solve_ms * 1e-3) / 1e12
    return {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBPS,
            "traffic": traffic, "traffic_source": traffic_source, "kernel": "mpcx::solve_kernel", "kernel_ms": solve_ms,
            "algorithmic_bytes_per_satellite": B,
            "note": "algorithmic bytes = 8(27K+7)+8 + 1680(K-1) per satellite-MPC-step (SURVEY 8d, two-kernel form) x satellites per "
                    "launch; duration = HIP events around solve_kernel on its launch stream; traffic = FETCH_SIZE+WRITE_SIZE of "
                    "profiles/ (workspace traffic: the kernel is bound by the latency / issue rate of one wave per satellite, not by "
                    "its algorithmic HBM bytes)",
            # what actually limits the kernel: fp64 vector arithmetic against the 78.6 TFLOP/s fp64 vector peak.  `achieved` =
            # the operations the launch EXECUTES by the committed SQ counters (64 lanes per wave instruction) / this run's kernel
            # time; `useful` = the ~18 kflop per node and interior-point iteration of the algorithm
            "valu_f64": {"achieved": tf(executed), "peak": F64_VALU_PEAK_TFLOPS, "unit": "TFLOP/s",
                         "frac": None if executed is None else tf(executed) / F64_VALU_PEAK_TFLOPS, "source": flop_source,
                         "useful": {"achieved": tf(useful), "frac": tf(useful) / F64_VALU_PEAK_TFLOPS,
                                    "note": "18 kflop per node and iteration x the iterations of the last launch"}}}


def host_pointer_rate(h, S, local_rank, reps=20):
    """the same step through the host-pointer entry point (numpy in / numpy out): H2D of the inputs and D2H of the results
    through the context's pinned staging inside the timed region -- the PCIe-inclusive figure of SURVEY 8(d), reported
    beside `value`, never as `value`"""
    from mpconstellation_amd import mpc_step_batch, _ffi

    import gc
    pauses = []
    t_gc = [0.0]

    def on_gc(phase, info):
        if phase == "start": t_gc[0] = time.perf_counter()
        else: pauses.append((time.perf_counter() - t_gc[0]) * 1e3)

    def timed(f):
        # two untimed calls (the first grows the context's staging pools and workspace), then `reps` timed ones; every call
        # is listed, with median and max beside the mean so that a stall can neither hide nor pass for the steady state.
        # Python's cyclic garbage collector is watched during the timed calls: with torch imported a full (generation 2)
        # collection of this process takes tens of milliseconds and lands inside whichever call triggers it
        # (profiles/r04/host_stall.txt).
        warm = []
        for _ in range(2):
            t0 = time.perf_counter(); f(); warm.append((time.perf_counter() - t0) * 1e3)
        ms = []
        pauses.clear(); gc.callbacks.append(on_gc)
        try:
            for _ in range(reps):
                t0 = time.perf_counter(); f(); ms.append((time.perf_counter() - t0) * 1e3)
        finally:
            gc.callbacks.remove(on_gc)
        return float(np.mean(ms)) * 1e-3, {"timed": [round(v, 3) for v in ms], "warmup": [round(v, 3) for v in warm],
                                           "median": round(float(np.median(ms)), 3), "max": round(float(np.max(ms)), 3),
                                           "python_gc_pauses_ms": [round(v, 2) for v in pauses if v >= 0.5]}
    dt, calls = timed(lambda: mpc_step_batch(h["xbar"], h["ubar"], h["tfbar"], h["consts"], h["r_des"], device=local_rank))
    # the same with the caller's arrays in page-locked memory (mpcx_host_alloc): DMA straight from / to them
    hp = {k: _ffi.pinned_copy(h[k], local_rank) for k in ("xbar", "ubar", "tfbar", "consts", "r_des")}
    dtp, callsp = timed(lambda: mpc_step_batch(hp["xbar"], hp["ubar"], hp["tfbar"], hp["consts"], hp["r_des"], device=local_rank,
                                               pinned_results=True))
    return {"value": S / dtp, "unit": "satellite-MPC-steps/s", "ms_per_call": dtp * 1e3, "calls_ms": callsp,
            "pageable": {"value": S / dt, "ms_per_call": dt * 1e3, "calls_ms": calls},
            "note": "mpcx_mpc_step_batch: one SCP iteration per call, H2D of xbar, ubar, tf, consts, r_des and D2H of x, u, nu, "
                    "tf, status inside the timed region (SURVEY 8d's PCIe-inclusive figure): caller arrays in page-locked memory "
                    "(mpcx_host_alloc); `pageable`: ordinary numpy arrays, staged through the context's pinned pool"}


def also_workload(name, steps, warmup, local_rank, note, with_host=False, flags=0):
    """one more BASELINE config measured in the same run under the driver's clock (its own Runner, steps, warmup)"""
    import torch
    S, K, n_scp = WORKLOADS[name]
    r = Runner(name, 0, 1, local_rank)
    r.opts.flags = flags
    e, sm = measure(r, steps, warmup, 1)
    st, it, kk = r.solver_stats()
    out = {"value": S * steps / e, "unit": "satellite-MPC-steps/s", "steps": steps, "warmup": warmup,
           "ms_per_step": e / steps * 1e3, "roofline": roofline(name, S, K, sm, it),
           "solver": {"converged": int(((st == 0) | (st == 7)).sum()), "of": S, "ipm_iterations_mean": float(it.mean()),
                      "ipm_iterations_max": int(it.max()), "kkt_max": float(kk.max())}, "note": note}
    if flags:
        # (the counters committed for the workload's own name are the default kernels'; the time-parallel kernel's are under
        #  <name>_tp -- profiles/collect.sh -- and nothing is echoed for any other flag set)
        out["roofline"].pop("valu_f64", None)
        if flags == 64:
            out["roofline"]["traffic"], out["roofline"]["traffic_source"] = measured_traffic(name + "_tp", "solve_kernel_tp")
            out["roofline"]["kernel"] = "mpcxtp::solve_kernel_tp"
        else:
            out["roofline"]["traffic"] = None; out["roofline"].pop("traffic_source", None)
    if n_scp > 1:
        out["scp_iterations_per_s"] = out["value"] * n_scp
    if with_host:
        out["host_pointer_entry"] = host_pointer_rate(r.host, S, local_rank)
    del r
    torch.cuda.empty_cache()
    return out


def closed_loop(S, local_rank, segments=2, time_parallel=False):
    """The metric's "MPC steps/sec (whole constellation)" for the loop the hot path sits in: ConstellationMPC.run_segments
    in the reference's test_mpc configuration (test_simulator.py:79-98: base_res 30, tf_horizon 2, two segments, r_des 1.5,
    truth model with drag + J2 at base_res 100).  One constellation-MPC-step = controller.update() for every satellite
    (reference rollout + 2 SCP iterations with re-rollout, control.py:170-235) + the truth propagation of the segment
    (simulator.py:58-65), host Python included, numpy arrays in and out."""
    from mpconstellation_amd import Satellite, ConstellationMPC
    from mpconstellation_amd.constellation import constellation_states
    st = constellation_states(S)
    make = lambda: [Satellite(s[:3].copy(), s[3:6].copy(), float(s[6])) for s in st]
    ConstellationMPC(make(), base_res=30, tf_horizon=2, tf_interval=1, r_des=1.5, sim_base_res=100, device=local_rank, time_parallel=time_parallel).run_segments(tf=2, num_segments=1)   # warm-up: workspaces, staging pools
    mpc = ConstellationMPC(make(), base_res=30, tf_horizon=2, tf_interval=1, r_des=1.5, sim_base_res=100, device=local_rank, time_parallel=time_parallel)
    t0 = time.perf_counter()
    mpc.run_segments(tf=2, num_segments=segments)
    dt = time.perf_counter() - t0
    ok = int(np.isin(mpc.last_status, (0, 7)).sum())
    t = mpc.timing
    return {"value": S * segments / dt, "unit": "satellite-MPC-steps/s (1 step = OptimalController.update + segment flight)",
            "satellites": S, "segments": segments, "s_per_segment": dt / segments, "scp_iterations_per_s": 2 * S * segments / dt,
            "converged_last_segment": ok, "of": int(mpc.last_status.size),
            "split_s": {k: round(v, 4) for k, v in t.items()}, "host_python_s": round(dt - sum(t.values()), 4)}


def api_devices8_overhead(local_rank, S=65536, K=30, ndev=8, calls=5):
    """Host time a multi-device call of the drop-in API adds AROUND the library calls: mpc_step_batch(devices=[d] * 8) at BASELINE
    configs[4]'s 65 536 satellites x 30 nodes with eight contexts of THIS one device (the eight-device execution itself is
    unmeasured on hardware; what is measured is the host's share: result set, slicing, threads) -- wall time of the Python call
    minus the span from the first library entry to the last library return (profiles/tools/devices8_overhead.py is the same
    measurement with the round-4 package beside it: 21.8 ms of np.concatenate then, profiles/r05/devices8_host_overhead.txt)."""
    import threading
    from mpconstellation_amd import _ffi, mpc_step_batch
    from mpconstellation_amd.constellation import constellation_states, normalize_batch, tangential_thrust
    from mpconstellation_amd.simulator import propagate_batch
    y0, consts = normalize_batch(constellation_states(S))
    xbar = np.empty((S, 7, K))
    for b in range(0, S, 8192):
        xbar[b:b + 8192] = propagate_batch(y0[b:b + 8192], 1.0, consts[b:b + 8192], (_ffi.CTRL_TANGENTIAL, np.array([0.5]), 0, None), K, device=local_rank)[0]
    ubar = np.ascontiguousarray(tangential_thrust(xbar, 0.5)); r_des = np.linalg.norm(xbar[:, :3, -1], axis=1); tf = np.ones(S)
    lib = _ffi.load(); inner = lib.mpcx_mpc_step_batch
    spans = []; lock = threading.Lock()

    def timed(*a):
        t0 = time.perf_counter(); rc = inner(*a); t1 = time.perf_counter()
        with lock: spans.append((t0, t1))
        return rc
    lib.mpcx_mpc_step_batch = timed
    rows = []; res = None
    try:
        for _ in range(calls + 2):
            res = None; spans.clear()
            t0 = time.perf_counter()
            res = mpc_step_batch(xbar, ubar, tf, consts, r_des, devices=[local_rank] * ndev)
            t1 = time.perf_counter()
            rows.append((1e3 * (t1 - t0), 1e3 * (max(x[1] for x in spans) - min(x[0] for x in spans))))
    finally:
        lib.mpcx_mpc_step_batch = inner
    ok = int((res.status == 0).sum())
    rows = rows[2:]
    return {"api_devices8_host_overhead_ms": float(np.mean([w - l for w, l in rows])), "wall_ms": float(np.mean([w for w, _ in rows])),
            "library_span_ms": float(np.mean([l for _, l in rows])), "satellites": S, "contexts": ndev, "converged": ok,
            "value": S / (np.mean([w for w, _ in rows]) * 1e-3),
            "note": "mpc_step_batch(devices=[0] * 8), numpy in / numpy out, eight contexts and host threads on ONE device: the device calls "
                    "serialise (unmeasured on eight devices); the overhead is what the host adds around them -- one result set, written in place"}


def spawn_ranks(args):
    """--gpus N without an outer launcher: start the N ranks as child processes (this parent never touches a GPU) and
    pass their output and exit code through."""
    port = 29500 + (os.getpid() % 2000)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ); env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", default=None, choices=sorted(WORKLOADS),
                    help=f"default: {DEFAULT_SINGLE} per GPU at every N (with N > 1 and --full also S8192_K30 per GPU, reported under `also`)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-also", action="store_true", help="skip the extra workloads, host-pointer and closed-loop measurements of a --full run")
    ap.add_argument("--cpu-sample", type=int, default=256, help="satellites solved by the CPU oracle")
    ap.add_argument("--solve-flags", type=int, default=0, help="mpcx_solve_opts.flags of the measured solves (64: the time-parallel kernel; profiling runs)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, everything else the line can carry: the host-pointer entry (value_pcie), the index launch "
                         "order, the other BASELINE workloads, the closed loop, the CPU oracle baseline and the trajectory error against it "
                         "(with N > 1: configs[4]'s 8192 satellites per GPU); --no-also / --no-cpu-baseline trim it")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the timed path computed in its last step as DIR/<name>.npy (float64)")
    args = ap.parse_args()

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        raise SystemExit(spawn_ranks(args))

    import torch
    import torch.distributed as dist
    rank = int(os.environ.get("RANK", "0")); world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks")
    single_dev = os.environ.get("MPCX_BENCH_SINGLE_DEVICE") == "1"   # rehearsal of the N>1 path on a 1-GPU box (gloo)
    if single_dev:
        local_rank = 0
    have_gpu = torch.cuda.is_available()
    if have_gpu: torch.cuda.set_device(local_rank)       # before the process group: RCCL binds its communicator to the current device
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo" if (single_dev or not have_gpu) else "nccl")
    if not have_gpu:
        raise SystemExit("bench.py needs an MI355X: libmpcx has no CPU fallback")
    workload = args.workload or DEFAULT_SINGLE

    run = Runner(workload, rank, world, local_rank)
    run.opts.flags = args.solve_flags
    S, K, n_scp = run.S, run.K, run.n_scp
    elapsed, solve_ms = measure(run, args.steps, args.warmup, world)
    status, iters, kkt = run.solver_stats()
    stats = torch.tensor([float(((status == 0) | (status == 7)).sum()), float(S)], dtype=torch.float64,
                         device="cpu" if (world > 1 and dist.get_backend() == "gloo") else "cuda")
    if world > 1: dist.all_reduce(stats)
    if args.dump_outputs:
        dump_outputs(run, status, iters, kkt, args.dump_outputs, rank, world)
    also_multi = None
    if args.full and world > 1 and not args.no_also and workload == DEFAULT_SINGLE:
        # BASELINE configs[4] (65 536 satellites over 8 GPUs = 8192 per GPU) by every rank in the same run, timed the same way
        # (barriers, slowest rank); the headline keeps the per-GPU work of the N = 1 line so that the N = 1, 2, 4, 8 values are
        # one weak-scaling curve
        run4 = Runner("S8192_K30", rank, world, local_rank)
        e4, sm4 = measure(run4, 5, 1, world)
        st4, it4, _ = run4.solver_stats()
        stats4 = torch.tensor([float(((st4 == 0) | (st4 == 7)).sum())], dtype=torch.float64, device=stats.device)
        dist.all_reduce(stats4)
        also_multi = {"S8192_K30": {"value": run4.S * world * 5 / e4, "unit": "satellite-MPC-steps/s", "steps": 5, "warmup": 1,
                                    "ms_per_step": e4 / 5 * 1e3, "satellites_per_gpu": run4.S, "satellites_total": run4.S * world,
                                    "solve_kernel_ms_rank0": sm4, "converged": int(stats4[0].item()), "of": run4.S * world,
                                    "note": "BASELINE configs[4]'s share per GPU (65 536 satellites on 8), all ranks, same run"}}
        del run4
        torch.cuda.empty_cache()

    if rank == 0:
        S_total = S * world
        value = S_total * args.steps / elapsed
        out = {
            "metric": "satellite-MPC-steps/sec (whole constellation; 1 step = discretize + constraint terms + solve per SCP iteration; inputs "
                      "and results resident in HBM -- value_pcie is the same step with H2D of the inputs and D2H of the results inside)",
            "value": value, "unit": "satellite-MPC-steps/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": workload + (f" (solve flags {args.solve_flags})" if args.solve_flags else ""), "satellites_per_gpu": S, "satellites_total": S_total, "nodes_K": K,
                       "scp_iterations_per_step": n_scp, "parallelism": f"satellite-sharded x{world}, no collective"},
            "roofline": roofline(workload, S, K, solve_ms, iters),
            "solver": {"converged": int(stats[0].item()), "of": int(stats[1].item()),
                       "ipm_iterations_mean": float(iters.mean()), "ipm_iterations_max": int(iters.max()),
                       "kkt_max": float(kkt.max())},
        }
        if n_scp > 1:
            out["scp_iterations_per_s"] = value * n_scp
        h = run.host
        # device results of the timed steps (first SCP iteration's inputs are the host arrays only when n_scp == 1)
        dev_res = (run.d_X.cpu().numpy(), run.d_U.cpu().numpy(), run.d_tfo.cpu().numpy(), status) if args.full and n_scp == 1 else None
        if args.full and world == 1 and not args.no_also:
            out["host_pointer_entry"] = host_pointer_rate(h, S if n_scp == 1 else S / n_scp, local_rank)
            # SURVEY 8(d)'s metric with H2D of the inputs and D2H of the results inside the timed region, ordinary numpy
            # arrays in and out (what the drop-in Optimizer passes): beside `value`, never instead of it
            out["value_pcie"] = out["host_pointer_entry"]["pageable"]["value"]
            # the default launch order is longest-first by the previous solve's iteration counts (consecutive steps pose
            # similar problems: the Runner cycles through reference-thrust variants); the plain index order beside it
            run.opts.flags = 1; run.solve_events = []
            ei, si = measure(run, max(2, args.steps // 2), 1, 1)
            run.opts.flags = 0
            out["index_launch_order"] = {"value": S * max(2, args.steps // 2) / ei, "ms_per_step": ei / max(2, args.steps // 2) * 1e3,
                                         "solve_kernel_ms": si}
        if args.full and world == 1 and not args.no_also and workload == DEFAULT_SINGLE:
            del run
            torch.cuda.empty_cache()
            out["also"] = {
                "S64_K30": also_workload("S64_K30", args.steps, args.warmup, local_rank,
                                         "BASELINE configs[1] (64 satellites: 64 of the chip's 1024 SIMDs busy), same run", with_host=True),
                "S64_K30_time_parallel": also_workload("S64_K30", args.steps, args.warmup, local_rank,
                                                       "the same 64 satellites on the time-parallel kernel (MPCX_SOLVE_TIME_PARALLEL: four segments of the horizon side by "
                                                       "side, a workgroup each; same iterations, not the default kernels' bits), same run", flags=64),
                "S4096_K100_scp2": also_workload("S4096_K100_scp2", 3, 1, local_rank,
                                                 "BASELINE configs[3]: K = 100, 2 SCP iterations with device re-rollout per step, same run"),
                "S8192_K30": also_workload("S8192_K30", 5, 1, local_rank,
                                           "one GPU's share of BASELINE configs[4] (65 536 satellites over 8 GPUs), same run"),
            }
            out["closed_loop"] = {f"S{n}": closed_loop(n, local_rank) for n in (64, 4096)}
            out["closed_loop"]["S64_time_parallel"] = closed_loop(64, local_rank, time_parallel=True)
            out["also"]["api_devices8"] = api_devices8_overhead(local_rank)
        if also_multi: out["also"] = also_multi
        if args.full and not args.no_cpu_baseline and world == 1:
            out["cpu_baseline"], err = cpu_baseline(h["xbar"], h["ubar"], h["tfbar"], h["consts"], h["r_des"], args.cpu_sample, dev_res)
            if err: out["trajectory_error_vs_cpu_oracle"] = err
        print(json.dumps(with_summary(out)), flush=True)
    if world > 1:
        dist.barrier(); dist.destroy_process_group()


CONTRACT_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
                 "data", "config")


def with_summary(out):
    """the line's secondary headline numbers in ONE short dict right behind the contract's keys -- ahead of the long per-call
    lists and notes, so that a reader (or a log tail cut off at some length) finds them without the rest"""
    g = lambda d, *ks: (g(d.get(ks[0], {}), *ks[1:]) if len(ks) > 1 else d.get(ks[0])) if isinstance(d, dict) else None
    rnd = lambda v: None if v is None else round(float(v), 3)
    summ = {"value_pcie": rnd(out.get("value_pcie")), "solve_kernel_ms": rnd(g(out, "roofline", "kernel_ms")),
            "roofline_frac": g(out, "roofline", "frac"), "cpu_baseline": rnd(g(out, "cpu_baseline", "value")),
            "cpu_baseline_all_cores": rnd(g(out, "cpu_baseline", "all_cores", "value"))}
    for k, v in (out.get("also") or {}).items():
        if isinstance(v, dict):
            summ["also." + k] = rnd(v.get("value"))
            km = g(v, "roofline", "kernel_ms")
            if km is not None: summ["also." + k + ".kernel_ms"] = rnd(km)
    if g(out, "also", "api_devices8", "api_devices8_host_overhead_ms") is not None:
        summ["also.api_devices8_host_overhead_ms"] = rnd(out["also"]["api_devices8"]["api_devices8_host_overhead_ms"])
    for k, v in (out.get("closed_loop") or {}).items():
        summ["closed_loop." + k] = rnd(v.get("value"))
    ordered = {k: out[k] for k in CONTRACT_KEYS if k in out}
    ordered["summary"] = {k: v for k, v in summ.items() if v is not None}
    for k in ("roofline", "cpu_baseline"):                 # the two objects the contract adds, then everything else
        if k in out: ordered[k] = out[k]
    ordered.update({k: v for k, v in out.items() if k not in ordered})
    return ordered


def cpu_quota():
    """CPUs' worth of run time the process's cgroup allows (cgroup v2 cpu.max, v1 cfs quota), None if unlimited / unknown"""
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        return None if q == "max" else float(q) / float(per)
    except Exception:
        pass
    for d in ("/sys/fs/cgroup/cpu", "/sys/fs/cgroup/cpu,cpuacct"):
        try:
            q = float(open(d + "/cpu.cfs_quota_us").read()); per = float(open(d + "/cpu.cfs_period_us").read())
            return None if q <= 0 else q / per
        except Exception:
            pass
    return None


def _cpu_worker(job):
    """one satellite-MPC-step on the CPU oracle (C discretize + numpy interior point); runs in a spawned worker"""
    sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle_lib as O
    import nlp_ipm as N
    x, u, tf, cst, rd = job
    d = O.discretize(x, u, tf, cst)
    P = N.MpcProblem(x, u, tf, cst[0], d, O.constraint_terms(x, u, cst[0]), {"r_des": rd})
    r = N.solve(P)
    return r["status"], r["X"], r["U"], r["tf"]


def cpu_baseline(xbar, ubar, tfbar, consts, r_des, n, dev_res=None):
    """The CPU oracle (oracle/: C discretize + numpy interior point) timed on ALL host cores (one worker process per core,
    satellites dealt out evenly) on the first n satellites of the same workload.  Reported baseline only; pyomo+ipopt are
    not installed on this image.  With the device results of the same satellites it also returns BASELINE.json's
    'trajectory error' against the stand-in for ipopt (the oracle): max and 99th percentile over the sample."""
    import multiprocessing as mp
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as O
    O.build()                                             # the C half, once, before the workers load it
    n = min(n, xbar.shape[0])
    # one single-threaded worker per host core of this GPU's share of the box: the benchmark pool gives a one-GPU job 16 of
    # the node's cores (its rule for worker pools; nproc is reported beside it, MPCX_CPU_WORKERS overrides), never more than
    # the process may run on
    cores = min(len(os.sched_getaffinity(0)), int(os.environ.get("MPCX_CPU_WORKERS", "16")))
    for var in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
        os.environ[var] = "1"                            # inherited by the spawned workers: no BLAS thread pools inside them
    jobs = [(xbar[i], ubar[i], float(tfbar[i]), consts[i], float(r_des[i])) for i in range(n)]
    with mp.get_context("spawn").Pool(cores) as pool:
        pool.map(_cpu_worker, jobs[:cores])               # workers import numpy / load the library outside the timed region
        t0 = time.perf_counter()
        res = pool.map(_cpu_worker, jobs, chunksize=max(1, n // (4 * cores)))
        dt = time.perf_counter() - t0
    ok = sum(int(r[0] in (0, 7)) for r in res)
    # ... and the same on EVERY core the process may run on (one process per host core, count stated), on a
    # sample scaled with the cores (4 satellites per worker, at least n)
    all_cores = None
    # (the cores the process may RUN on: its affinity mask cut down to its cgroup's CPU quota -- on the benchmark pool a one-GPU job
    #  sees all 256 cores of the node in its mask and is throttled to a share of them; 256 workers on that share measured 123
    #  steps/s against 197 with 16, gpurun r5f)
    quota = cpu_quota()
    avail = min(len(os.sched_getaffinity(0)), int(os.environ.get("MPCX_CPU_WORKERS_ALL", "512")))
    if quota is not None: avail = min(avail, max(1, int(quota + 0.5)))
    if avail <= cores:
        all_cores = {"value": None, "cores": avail, "sample": f"not run: the process may use {avail} core(s) (affinity {len(os.sched_getaffinity(0))}, cgroup CPU quota "
                                                                 f"{'none' if quota is None else round(quota, 2)}), no more than the {cores} of the figure above"}
    if avail > cores:
        n_all = min(xbar.shape[0], max(n, 4 * avail))
        jobs_all = [(xbar[i], ubar[i], float(tfbar[i]), consts[i], float(r_des[i])) for i in range(n_all)]
        with mp.get_context("spawn").Pool(avail) as pool:
            pool.map(_cpu_worker, jobs_all[:avail], chunksize=1)
            t0 = time.perf_counter()
            res_all = pool.map(_cpu_worker, jobs_all, chunksize=max(1, n_all // (8 * avail)))
            dt_all = time.perf_counter() - t0
        all_cores = {"value": n_all / dt_all, "unit": "satellite-MPC-steps/s", "cores": avail,
                     "sample": f"first {n_all} satellites, one single-threaded worker process per core the process may run on ({avail} of nproc = "
                               f"{os.cpu_count()}), {sum(int(r[0] in (0, 7)) for r in res_all)}/{n_all} converged, {dt_all:.1f} s wall"}
    ex, eu, et = [], [], []
    if dev_res is not None:
        for i, r in enumerate(res):
            if r[0] == 0 and dev_res[3][i] == 0:
                ex.append(np.abs(dev_res[0][i] - r[1]).max()); eu.append(np.abs(dev_res[1][i] - r[2]).max())
                et.append(abs(dev_res[2][i] - r[3]))
    ref_timing = None
    rt = os.path.join(ROOT, "tests", "golden", "reference_cpu_timing.json")
    if os.path.exists(rt):
        j = json.load(open(rt))
        ref_timing = {"where": "build container, not this box (the reference cannot travel; tests/golden/time_reference.py)",
                      "host": j.get("host"), "nproc": j.get("nproc"), "seconds_per_satellite": j.get("results"),
                      "what": j.get("what"), "not_timed": j.get("not_timed")}
    base = {"value": n / dt, "unit": "satellite-MPC-steps/s", "cores": cores, "kind": "port", "all_cores": all_cores, "reference_discretize": ref_timing,
            "sample": f"first {n} satellites of the workload, oracle/ (C discretize + numpy IPM), one single-threaded worker process "
                      f"per host core of this GPU's share ({cores} of nproc = {os.cpu_count()}), {ok}/{n} converged, "
                      f"{dt:.1f} s wall = {dt * cores:.0f} core-seconds"}
    err = None
    if ex:
        q = lambda v: {"max": float(np.max(v)), "p99": float(np.percentile(v, 99))}
        err = {"x": q(ex), "u": q(eu), "tf": q(et), "satellites": len(ex), "stated_tolerance": 5e-6,
               "note": "normalised units; both sides converged to ipopt's scaled error 1e-8 on a flat objective (w_tr = 0.002); "
                       "the reference's ipopt itself is not available on this image (parity unpinned, DESIGN.md section 2); "
                       "tests/test_solve_xcheck_gpu.py compares the device with independent scipy solutions of the same NLP"}
    return base, err


if __name__ == "__main__":
    main()
