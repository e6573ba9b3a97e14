"""The one-wave factorisation loop (solve_riccati.hpp, riccati_factor) is specialised by node position: the terminal node K-1
and node 0 are peeled off, the loop body runs K-2 .. 1.  Held bit for bit against the two-wave kernel (riccati_factor2, which
has no such specialisation) at the horizons where the body runs one, two or three times and on the paths the peeling touches:
refinement passes (the factor record's Pt), stiff stage terms, factorisation breakdowns retried with a larger delta_w, and a
batch above 1024 satellites (the size that runs the one-wave kernel by default)."""
import numpy as np
import pytest

from test_full_size_gpu import workload

pytestmark = pytest.mark.gpu

F = ("X", "U", "NU", "tf", "kkt", "status", "iters", "n_regularised", "first_regularised")
OPTIMAL_CONTROLLER = {"eps_r": 1e-6, "eps_vr": 1e-16, "tf_max": 1.0}      # stiff terminal windows: refinement passes
THRUST_LIMITED = {"u_lim": [0, 0.3]}                                       # thrust ball active: regularised iterations


def _one_vs_two(S, K, opts):
    from mpconstellation_amd import mpc_step_batch
    xbar, ubar, consts, r_des = workload(4096, K, first=0, count=S)
    tf = np.ones(S)
    one = mpc_step_batch(xbar, ubar, tf, consts, r_des, options=opts, flags=16, regularised=True)
    two = mpc_step_batch(xbar, ubar, tf, consts, r_des, options=opts, flags=32, regularised=True)
    assert np.isin(two.status, (0, 7)).all()
    for f in F:
        assert np.array_equal(getattr(one, f), getattr(two, f)), (S, K, opts, f)


@pytest.mark.parametrize("K", [3, 4, 5])
def test_short_horizons(K):
    # K = 3, 4, 5: the loop body (nodes K-2 .. 1) runs one, two and three times between the two peeled nodes
    _one_vs_two(32, K, {})


@pytest.mark.parametrize("K", [3, 4, 30])
def test_refinement_passes(K):
    _one_vs_two(64, K, OPTIMAL_CONTROLLER)


@pytest.mark.parametrize("K", [3, 4, 30])
def test_thrust_limited_regularised(K):
    _one_vs_two(64, K, THRUST_LIMITED)


def test_large_batch_one_wave():
    # above 1024 satellites: the one-wave kernel; a satellite's result does not depend on its batch companions
    from mpconstellation_amd import mpc_step_batch
    S, n = 1280, 64
    xbar, ubar, consts, r_des = workload(4096, 30, first=0, count=S)
    big = mpc_step_batch(xbar, ubar, np.ones(S), consts, r_des, flags=16, regularised=True)
    assert np.isin(big.status, (0, 7)).all()
    for first in (0, S - n):
        sl = slice(first, first + n)
        two = mpc_step_batch(xbar[sl].copy(), ubar[sl].copy(), np.ones(n), consts[sl].copy(), r_des[sl].copy(), flags=32,
                             regularised=True)
        for f in F:
            assert np.array_equal(getattr(big, f)[sl], getattr(two, f)), (first, f)
