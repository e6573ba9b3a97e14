"""discretize_kernel's step-size controller and its shared evaluations against the CPU oracle, where each of their paths is taken.

The kernel evaluates the controller's pow only where its value decides the next step (rk_accepted_h_abs, csrc/mpcx_device.hpp:
not on an interval's last step, not where the factor is the maximum, not where the next step is max_step anyway), shares the time
part of the last two RK45 stages, and lets the node of an accepted step take the last stage's evaluation when the whole wave
accepted.  The benchmark's regime (max_step = 1e-2, no rejections) never needs the pow and never leaves the shared paths; the
first test here is where it does both: long intervals with max_step = 1, rejected steps in the same wave as accepted ones.
Host side of the controller: tests/test_rk_step_factor_host.py."""
import functools
import os

import numpy as np
import pytest

import drag_cases as D
import oracle_lib as O

pytestmark = pytest.mark.gpu
RTOL = 1e-10                     # tests/test_discretize_gpu.py
RTOL_LONG = 1e-8                 # tests/test_discretize_gpu.py::test_long_intervals_exercise_the_pivoting (Phi's condition number 1e3 .. 2e4)
KEYS = ("A", "Bp", "Bn", "Sigma", "xi")
CST = np.array([39.47841760435743, 0.92, 1.08262668E-3, 46.5, 0.0873, 1e-12, 6.9e6, 3.7e-17])


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _inputs(seed, S, K, Ku, tf_range, thrust):
    """S satellites on tangential climbs from different orbits (the nodes of the oracle's rollout), seeded random thrust tables of
    Ku columns and final times"""
    rng = np.random.default_rng(seed)
    tan = O.make_ctrl(O.CTRL_TANGENTIAL, (0.3, 0, 0))
    xs, us, tfs = [], [], []
    for s in range(S):
        v = 2 * np.pi * (1 + 0.1 * rng.random())
        y0 = np.array([1, 0, 0, 0, v * np.cos(0.3 * s), v * np.sin(0.3 * s), 1.0])
        tf = rng.uniform(*tf_range)
        x, rc, _ = O.propagate(y0, tf, CST, tan, K)
        assert rc == 0
        xs.append(x); us.append(rng.normal(size=(3, Ku)) * thrust); tfs.append(tf)
    return np.stack(xs), np.stack(us), np.array(tfs)


def _oracle(x, u, tf, max_step, flags=0):
    """per satellite: the oracle's arrays, accepted steps and rejected attempts per interval (RK45: two evaluations to start an
    interval, six per attempt)"""
    outs = [O.discretize(x[s], u[s], float(tf[s]), CST, flags, max_step=max_step) for s in range(len(tf))]
    assert all(o["status"] == 0 for o in outs)
    accepted = np.concatenate([o["node_counts"] - 1 for o in outs])
    attempts = np.concatenate([(o["node_nfev"] - 2) // 6 for o in outs])
    return outs, accepted, attempts - accepted


@functools.lru_cache(None)
def rejecting_case():
    x, u, tf = _inputs(2024, 7, 4, 13, (0.8, 2.5), 0.5)
    return (x, u, tf) + _oracle(x, u, tf, 1.0)


@functools.lru_cache(None)
def benchmark_regime_case():
    x, u, tf = _inputs(99, 3, 12, 12, (0.5, 1.5), 0.5)
    return (x, u, tf) + _oracle(x, u, tf, 1e-2)


def _device_stages(x, u, tf, max_step, Ks=None, flags=0):
    import dev_solve
    S = x.shape[0]
    stage, st = dev_solve.discretize_stages(x, u, tf, np.tile(CST, (S, 1)), Ks=Ks, Kus=None if Ks is None else Ks, flags=flags, max_step=max_step)
    assert (st == 0).all(), st
    return [dev_solve.unpack_stage(stage, s, int(x.shape[2] if Ks is None else Ks[s])) for s in range(S)]


def _compare(got, ref, rtol, what):
    worst = 0.0
    for s, (g, o) in enumerate(zip(got, ref)):
        for k in KEYS:
            assert g[k].shape == o[k].shape, (what, s, k)
            e = relerr(g[k], o[k])
            worst = max(worst, e)
            print(f"{what}: satellite {s} {k}: relative error {e:.3g}")
    assert worst < rtol, (what, worst)
    return worst


def test_rejections_and_pow_in_mixed_waves():
    """S = 7, K = 4: 21 intervals in three waves of eight groups, the last with five live ones; thrust tables of 13 columns (not K),
    tf in [0.8, 2.5], max_step = 1: intervals of a quarter to most of an orbit, on which the controller rejects steps and, without
    a max_step to run into, nearly every accepted step needs its pow.  First on the CPU: at least three intervals reject a step,
    a wave holds a rejecting interval beside one that does not (the wave then leaves the shared node path while some of its
    groups accept), and the inputs sit on no step-acceptance knife edge -- with x moved by 1e-13 the oracle takes the same steps."""
    x, u, tf, ref, accepted, rejected = rejecting_case()
    assert (rejected > 0).sum() >= 3, rejected
    waves = [rejected[i:i + 8] for i in range(0, len(rejected), 8)]
    assert any((w > 0).any() and (w == 0).any() for w in waves), rejected
    _, accepted2, rejected2 = _oracle(x * (1 + 1e-13 * np.random.default_rng(1).standard_normal(x.shape)), u, tf, 1.0)
    assert (accepted2 == accepted).all() and (rejected2 == rejected).all()
    print(f"accepted steps per interval {accepted.tolist()}, rejected attempts {rejected.tolist()}")
    _compare(_device_stages(x, u, tf, 1.0), ref, RTOL_LONG, "rejecting")


def test_benchmark_regime_small():
    """S = 3, K = 12, max_step = 1e-2: the benchmark's regime -- every interval starts small, grows by the maximal factor, runs at
    max_step and ends on a clipped step; no rejection, no pow"""
    x, u, tf, ref, accepted, rejected = benchmark_regime_case()
    assert (rejected == 0).all() and (accepted >= 4).all(), (accepted, rejected)
    _compare(_device_stages(x, u, tf, 1e-2), ref, RTOL, "benchmark regime")


def test_one_interval_and_ragged_batch():
    """S = 1 with K = 2 (one live group in the only wave), and a ragged launch with Ks = (2, 5, 3): slots past a satellite's last
    interval shadow it"""
    x, u, tf, *_ = benchmark_regime_case()
    one = slice(0, 1)
    x2 = np.ascontiguousarray(x[one, :, :2]); u2 = np.ascontiguousarray(u[one, :, :2])
    ref, _, rejected = _oracle(x2, u2, tf[one], 1e-2)
    _compare(_device_stages(x2, u2, tf[one], 1e-2), ref, RTOL, "S = 1, K = 2")
    Ks = np.array([2, 5, 3], dtype=np.int32)
    xr, ur = np.full((3, 7, 5), np.nan), np.full((3, 3, 5), np.nan)
    refs = []
    for s, k in enumerate(Ks):
        xr[s, :, :k], ur[s, :, :k] = x[s, :, :k], u[s, :, :k]
        refs.append(_oracle(xr[s:s + 1, :, :k], ur[s:s + 1, :, :k], tf[s:s + 1], 1e-2)[0][0])
    _compare(_device_stages(xr, ur, tf, 1e-2, Ks=Ks), refs, RTOL, "ragged")


def test_drag_atmosphere_and_rk23(golden_dir):
    """one drag + atmosphere + J2 input (tests/drag_cases.py: the batch under the general model, RK45) and the RK23 golden of the
    reference: the other instantiations of the kernel take the same controller and the same shared evaluations"""
    from mpconstellation_amd import Discretizer, Simulator
    from mpconstellation_amd.constants import Constants
    from test_drag_oracle_gpu import discretizer, worst_against_oracle
    b = D.batch()
    out = discretizer(b["const"][0], "general", "rk45", True).discretize_batch(b["x"], b["u"], b["tf"], b["const"])
    assert (out[5] == 0).all(), out[5]
    worst = max(worst_against_oracle({k: out[i][s] for i, k in enumerate(KEYS)}, b["x"][s], b["u"][s], b["tf"][s], b["const"][s], "general", "rk45", True, s)
                for s in range(b["x"].shape[0]))
    print(f"drag + atmosphere: worst relative error {worst:.3g}")
    g = np.load(os.path.join(golden_dir, "rk23_discretize.npz"))
    d = Discretizer(Constants(*g["const"]))
    d.ivp_solver = "RK23"
    name = str(g["cases"][0])
    got = d.discretize(Simulator.satellite_dynamics, g[f"x_{name}"], g[f"u_{name}"], float(g[f"tf_{name}"]))
    for a, k in zip(got, KEYS):
        e = relerr(a, g[f"{k}_{name}"])
        print(f"RK23 {name} {k}: relative error {e:.3g}")
        assert e < RTOL, (name, k, e)
