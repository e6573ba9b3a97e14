"""Seven _dev forms of the listed-pair family were run by the timing tools alone: mpcx_collision_probability_dev,
mpcx_collision_probability_window_dev, mpcx_collision_window_sensitivity_dev, mpcx_encounter_window_dev, mpcx_avoidance_dev,
mpcx_avoidance_window_dev and mpcx_avoidance_joint_dev.  Each is held here to its host-pointer form bit for bit: the host form
stages the same arrays and enqueues the same kernels, so nothing may differ, whatever the caller's workspace and result buffers held
before (NaN, 1e300) and whether the optional outputs are asked for or NULL.

Inputs: the stored `figures` scene of tests/golden/encounter_parent_bits.npz (the slow pair as a pair of one constellation and as
satellite against catalogue) and, for the joint call, its `loops` scene (three satellites, rows that share one).  Device buffers are
torch tensors; compared are the integer views of every result."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import encounter_abi as A
from make_encounter_parent_bits import bits

pytestmark = pytest.mark.gpu

FIGURES = {
    "mpcx_collision_probability": {},
    "mpcx_collision_probability_window": {},
    "mpcx_collision_window_sensitivity": {},
    "mpcx_encounter_window": dict(max_half=np.full(1, 2000.0), nsigma=8.0, levels=3),
    "mpcx_avoidance": dict(P=None, cat_P=None, target=200.0),
    "mpcx_avoidance_window": dict(target_p=1e-3, tol=1e-6, max_eval=40),
}
CASES = [(name, form) for name in FIGURES for form in ("pair", "cat")] + [("mpcx_avoidance_joint", "loops")]


def scene(name, form):
    return A.three_satellites() if form == "loops" else dict(A.slow_pair(form), **FIGURES[name])


@pytest.mark.parametrize("name,form", CASES)
def test_dev_form_has_the_bits_of_the_host_form(name, form):
    import torch
    sc = scene(name, form)
    spec = A.results_of(name, sc)
    for optional in (True, False):
        host = A.with_results(name, sc, optional)
        assert A.call_host(name, host) == 0, A.last_error()
        statuses = np.concatenate([host[k].ravel() for k in spec if k.endswith("status")])
        assert (statuses == 0).all(), (name, form, statuses)              # a real answer, not a row of NaN
        for fill in (float("nan"), 1e300):
            d = A.on_device(sc)
            for k, (shape, dt, opt) in spec.items():
                d[k] = None if opt and not optional else torch.full(shape, fill if dt == np.float64 else -7, dtype=getattr(torch, np.dtype(dt).name), device="cuda:0")
            wsb = A.workspace_bytes(name, sc)
            assert wsb % 8 == 0
            d["workspace"] = torch.full((wsb // 8,), fill, dtype=torch.float64, device="cuda:0") if wsb else None
            assert A.call_dev(name, d) == 0, A.last_error()
            torch.cuda.synchronize()
            for k in spec:
                if d[k] is not None:
                    got = d[k].cpu().numpy()
                    assert got.dtype == host[k].dtype and np.array_equal(bits(got), bits(host[k])), (name, form, k, optional, fill)
