"""profiling helper of the Monte Carlo collision probability (csrc/collision_mc.hip): the models' own gaps and the call's time.
  gaps    the planted scenes of tests/collision_mc_scenes.py at N = 2^LOG2 samples beside the linearised figures on the same inputs
          (conjunction.covariance with q = 0, then collision_probability_window or collision_probability): the sampled START + ENTRIES
          against the rule's, the START columns, P_HIT against the short-encounter Pc, the excess of the re-entry scene.  A gap is
          what the run resolves beyond 4 of its own standard errors, else 0; tests/collision_mc_scenes.py holds 3 x these.
  checks  the sample covariance of the thrusting arc's last node against covariance_thrust's, with and without execution errors
          (tests/test_collision_mc_gpu.py's statistic at its N)
  times   mpcx_collision_probability_mc_dev, one row of two objects on one orbit, N = 2^LOG2, at K = 30 and K = 100, by HIP events on
          its stream: warmed up WARM times, timed REPS times, median, minimum and maximum.  The shares of the sampler, the flight and
          the scan come from a kernel trace of the same run taken separately (rocprofv3 --kernel-trace --stats around `times`).
usage: collision_mc_timing.py [gaps] [checks] [times] [--log2 20] [--reps 5]"""
import ctypes as C, os, statistics, sys
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import collision_reference as CR
import collision_mc_scenes as SC

args = sys.argv[1:]
LOG2 = int(args[args.index("--log2") + 1]) if "--log2" in args else 20
REPS = int(args[args.index("--reps") + 1]) if "--reps" in args else 5
WARM = 1
what = [a for a in args if a in ("gaps", "checks", "times")] or ["gaps", "checks", "times"]
N = 1 << LOG2

import torch                                                           # (its HIP runtime has to be the first one initialised in the process)
torch.cuda.is_available()
from mpconstellation_amd import _ffi, conjunction as cj


def resolved(diff, se):
    return abs(diff) if abs(diff) > 4.0 * se else 0.0


def window_figures(sc, half, N, scan, seed=1):
    P = cj.covariance(sc["Y"], sc["units"], sc["span"], sc["consts"], sc["P0"])
    win = cj.collision_probability_window(sc["pairs"], sc["radius"], sc["Y"], sc["units"], sc["span"], P, half, panels=sc["panels"])
    mc = cj.collision_probability_mc(sc["pairs"], sc["radius"], sc["Y"], sc["U"], sc["units"], sc["span"], sc["consts"], sc["P0"], half, N, seed=seed,
                                     scan=scan)
    assert win.status.tolist() == [0] and mc.status.tolist() == [0], (win.status, mc.status)
    return P, win, mc


if "gaps" in what:
    print(f"gaps at N = 2^{LOG2} = {N} samples (seed 1)", flush=True)
    for name, sc, scan in (("slow pair", SC.slow_pair(), 64), ("re-entry pair", SC.reentry_pair(), 128),
                           ("re-entry pair at sigmas of 2 m and 0.002 m/s (R / sigma = 18: outside the rule's quadrature)", SC.reentry_pair(sig_r=2.0, sig_v=0.002), 128)):
        P, win, mc = window_figures(sc, sc["half_window"], N, scan)
        rule, samp = win.start[0] + win.entries[0], mc.start[0] + mc.entries[0]
        se_start = np.sqrt(mc.start[0] * (1.0 - mc.start[0]) / mc.n_ok[0])
        print(f"  {name} (scan {scan}, panels {sc['panels']}, window {mc.window[0]}):", flush=True)
        print(f"    rule     START {win.start[0]:.6e} ENTRIES {win.entries[0]:.6e} sum {rule:.6e}")
        print(f"    sampled  START {mc.start[0]:.6e} ENTRIES {mc.entries[0]:.6e} sum {samp:.6e} SE_BOUND {mc.se_bound[0]:.3e}  P_HIT {mc.p_hit[0]:.6e} "
              f"SE_HIT {mc.se_hit[0]:.3e} EXCESS {mc.excess[0]:.6e} = {mc.excess[0] / max(mc.se_bound[0], 1e-300):.1f} SE_BOUND  counts {mc.counts[0].tolist()}")
        print(f"    sampled - rule: sum {samp - rule:+.3e} ({(samp - rule) / max(mc.se_bound[0], 1e-300):+.2f} SE_BOUND) -> gap {resolved(samp - rule, mc.se_bound[0]):.3e};  "
              f"START {mc.start[0] - win.start[0]:+.3e} ({(mc.start[0] - win.start[0]) / max(se_start, 1e-300):+.2f} SE) -> gap "
              f"{resolved(mc.start[0] - win.start[0], se_start):.3e}", flush=True)
    sc = SC.fast_pair()
    P = cj.covariance(sc["Y"], sc["units"], sc["span"], sc["consts"], sc["P0"])
    col = cj.collision_probability(sc["pairs"], sc["radius"], sc["Y"], sc["units"], sc["span"], P)
    ref, rst = CR.collision_probability(sc["pairs"], (sc["Y"], sc["units"], sc["span"], P, sc["radius"], None))
    half = cj.encounter_half_window(col, sc["radius"].sum())
    mc = cj.collision_probability_mc(sc["pairs"], sc["radius"], sc["Y"], None, sc["units"], sc["span"], sc["consts"], sc["P0"], half, N, seed=1, scan=64)
    assert col.status.tolist() == [0] and mc.status.tolist() == [0]
    print(f"  fast pair (scan 64, half window {half[0]:.4f} s): short-encounter Pc {col.pc[0]:.6e} (restated {ref[0, 0]:.6e}), sigma {col.sigma[0]} m, "
          f"R / sigma_2 {sc['radius'].sum() / col.sigma[0, 1]:.3f}, miss {col.miss[0]:.1f} m", flush=True)
    print(f"    sampled  P_HIT {mc.p_hit[0]:.6e} SE_HIT {mc.se_hit[0]:.3e} START {mc.start[0]:.3e} ENTRIES {mc.entries[0]:.6e} counts {mc.counts[0].tolist()}")
    print(f"    sampled - Pc {mc.p_hit[0] - col.pc[0]:+.3e} ({(mc.p_hit[0] - col.pc[0]) / mc.se_hit[0]:+.2f} SE) -> gap {resolved(mc.p_hit[0] - col.pc[0], mc.se_hit[0]):.3e}",
          flush=True)

if "checks" in what:
    Nc = 8192
    a = SC.thrust_arc(8)
    pairs = np.array([[0.0, 0.0, 0.0, 0.5 * a["span"][0, 1]]])
    L, Tu = a["units"][0]
    d = 1.0 / np.array([L] * 3 + [L / Tu] * 3)
    Pt = cj.covariance_thrust(a["Y"], a["units"], a["span"], a["consts"], a["P0"], a["U"], SC.EXEC)
    ref = Pt[0, -1] * d[:, None] * d[None, :]
    for label, ex in (("with execution errors", SC.EXEC), ("execution=None", None)):
        mc = cj.collision_probability_mc(pairs, 1.0, a["Y"], a["U"], a["units"], a["span"], a["consts"], a["P0"], 10.0, Nc, seed=2, scan=1, execution=ex,
                                         return_trajectories=True)
        x = mc.Y_samples[0, 0, :, :6, -1]
        got = np.cov(x.T)
        print(f"  thrusting arc K 8, N {Nc}, {label}: worst entry error over the largest entry {np.abs(got - ref).max() / np.abs(ref).max():.4e} "
              f"(bound {5.0 * np.sqrt(2.0 / Nc) + 3.0 * 5.83e-4:.4e})", flush=True)

if "times" in what:
    lib = _ffi.load(); ctx = _ffi.context(0)
    dev = torch.device("cuda", 0)
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    T = lambda a, dt=torch.float64: torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    E = lambda shape, dt=torch.float64: torch.empty(shape, dtype=dt, device=dev)
    print(f"times: one row, N = 2^{LOG2}, scan 64, default max_flights, {WARM} warm-up, {REPS} timed", flush=True)
    for K in (30, 100):
        R0 = 7.0e6
        span = (0.0, 2.0 * np.pi / np.sqrt(CR.MU_EARTH / R0 ** 3))
        u, v = np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0])
        ya, ua = CR.circular_through(R0 * u, v, 0.5 * span[1], K, span)
        th = -60.0 / R0
        yb, ub = CR.circular_through(R0 * (np.cos(th) * u + np.sin(th) * v), -np.sin(th) * u + np.cos(th) * v, 0.5 * span[1], K, span)
        Y, units, spans = np.stack([ya, yb]), np.stack([ua, ub]), np.array([span, span])
        ins = [T(x) for x in (np.array([[0.0, 1.0, 60.0, 0.5 * span[1]]]), Y, units, spans, SC.scale_constants(units[:, 0]),
                              np.broadcast_to(np.diag([40.0 ** 2] * 3 + [0.01 ** 2] * 3), (2, 6, 6)), np.array([10.0, 15.0]), np.array([0.4 * span[1]]))]
        counts, out, status = E((1, _ffi.NMCC), torch.int64), E((1, _ffi.NMC)), E(1, torch.int32)
        ws = E(lib.mpcx_collision_probability_mc_workspace_bytes(1, 2, K, 0, 0, N, 0), torch.uint8)
        call = lambda: lib.mpcx_collision_probability_mc_dev(ctx, 1, p(ins[0]), 2, K, None, p(ins[1]), None, p(ins[2]), p(ins[3]), p(ins[4]), 0, 1e-3,
                                                             p(ins[5]), None, None, p(ins[6]), 0, 0, None, None, None, None, None, None, None, p(ins[7]),
                                                             64, N, 1, 0, p(counts), p(out), p(status), None, None, None, p(ws), st)
        ms = []
        for i in range(WARM + REPS):
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            assert call() == 0, lib.mpcx_last_error(ctx)
            e1.record(); torch.cuda.synchronize()
            if i >= WARM:
                ms.append(e0.elapsed_time(e1))
        o = out.cpu().numpy()[0]
        print(f"  K {K:3d}: mpcx_collision_probability_mc_dev median {statistics.median(ms):9.2f} ms  min {min(ms):9.2f}  max {max(ms):9.2f}  ({len(ms)} runs); "
              f"workspace {ws.numel() / 2 ** 20:.0f} MiB; {2 * N / statistics.median(ms) / 1e3:.2f} M flights/s; P_HIT {o[0]:.5f} +- {o[1]:.5f}, status "
              f"{status.cpu().numpy().tolist()}, counts {counts.cpu().numpy()[0].tolist()}", flush=True)
        del ws
        torch.cuda.empty_cache()
