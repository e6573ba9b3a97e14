"""The solve kernels give bit for bit what they gave before the driver's iteration (solve_driver.hpp, ipm_iterate) was taken
out of solve_satellite and its loop state, counts and options moved to LDS: X, U, NU, tf, status, iterations, kkt and the
regularisation counts of every case of tests/golden/make_solve_driver_parent_bits.py -- the shortest horizon, a ragged batch
across the 32-node boundary with a refused row, K = 64 / 65 / 70 with refinement, n_refine = 0 / 1 / 2, regularised iterations,
and one case through each of the five kernels -- against tests/golden/solve_driver_parent_bits.npz, which that script recorded on
an MI355X from the library of the commit before the change."""
import os
import sys

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_solve_driver_parent_bits as G

pytestmark = pytest.mark.gpu
NAMES = list(G.CASES) + ["ragged"]
_recorded = {}


def recorded():
    if not _recorded:
        with np.load(os.path.join(GOLDEN, "solve_driver_parent_bits.npz")) as z:
            _recorded.update({k: z[k] for k in z.files})
    return _recorded


def test_every_case_is_recorded():
    assert sorted(recorded()) == sorted(f"{name}.{f}" for name in NAMES for f in G.FIELDS)


@pytest.mark.parametrize("name", NAMES)
def test_bits_of_the_parent(name):
    res = G.run_ragged() if name == "ragged" else G.run_case(name)
    for f in G.FIELDS:
        now, then = np.asarray(getattr(res, f)), recorded()[f"{name}.{f}"]
        assert now.shape == then.shape and now.dtype == then.dtype, (name, f)
        if not np.array_equal(now, then):
            print(f"{name}.{f}: {np.count_nonzero(now != then)} of {now.size} entries differ, max |d| {np.abs(now.astype(float) - then.astype(float)).max():.3e}")
        assert np.array_equal(now, then), (name, f)
