"""The solve kernels give bit for bit what they gave before the refinement residual (solve_phases.hpp, reduced_residual) went to two
lanes per node in passes of 32 nodes and border_solve formed its right-hand side one row per lane: X, U, NU, tf, status, iterations,
kkt and the regularisation counts of every case of tests/golden/make_refine_parent_bits.py -- stiff terminal windows, which refine
in most iterations, at K = 3, 4, 31, 32, 33 and 63, a ragged batch of 3 / 31 / 32 / 33 / 64 / 65 nodes, n_refine = 2, the linearised
tangential pair, a fixed final time, a thrust limit whose regularised iterations skip the refinement, and the K = 30 case through
each of the five kernels -- against tests/golden/refine_parent_bits.npz, which that script recorded on an MI355X from the library of
the commit before the change (asserting there that every case converged and that a refinement pass ran in it)."""
import os
import sys

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_refine_parent_bits as G

pytestmark = pytest.mark.gpu
_recorded = {}


def recorded():
    if not _recorded:
        with np.load(os.path.join(GOLDEN, "refine_parent_bits.npz")) as z:
            _recorded.update({k: z[k] for k in z.files})
    return _recorded


def test_every_case_is_recorded():
    assert sorted(recorded()) == sorted(f"{name}.{f}" for name in G.NAMES for f in G.FIELDS)


@pytest.mark.parametrize("name", G.NAMES)
def test_bits_of_the_parent(name):
    res = G.run(name)
    for f in G.FIELDS:
        now, then = np.asarray(getattr(res, f)), recorded()[f"{name}.{f}"]
        assert now.shape == then.shape and now.dtype == then.dtype, (name, f)
        if not np.array_equal(now, then):
            print(f"{name}.{f}: {np.count_nonzero(now != then)} of {now.size} entries differ, max |d| {np.abs(now.astype(float) - then.astype(float)).max():.3e}")
        assert np.array_equal(now, then), (name, f)
