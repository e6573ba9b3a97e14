"""The factorisation's LDS arrays are laid out for wide reads (solve_riccati.hpp: Pn with row stride 8, WlLi transposed, rows
fetched by lds_ld7).  That moves operands, not arithmetic: every build must still give, bit for bit, what the library gave
before the change.  tests/golden/factor_parent_bits.npz holds inputs and results written by that older library
(tests/golden/make_factor_parent_bits.py, which also lists the cases): the default kernel selection (LDS-resident and two-wave
builds at these sizes), the one-wave kernel the benchmark runs (MPCX_SOLVE_ONE_WAVE = 16) and, where K >= 24, the time-parallel
kernel (64) -- on the horizons where the loop body runs once and twice, the benchmark constellation, a ragged batch, option sets
with refinement passes (the factor record keeps Pt) and stiff stage terms, and a thrust limit below the reference thrust
(regularised iterations: a breakdown re-enters the factorisation)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_factor_parent_bits as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parent(golden_dir):
    return np.load(os.path.join(golden_dir, M.NAME))


@pytest.mark.parametrize("name", list(M.CASES))
def test_bits_of_the_parent_build(parent, name):
    S, K, Ks, opts = M.CASES[name]
    xbar, ubar, consts, r_des = (parent[f"{name}.{k}"] for k in ("xbar", "ubar", "consts", "r_des"))
    assert xbar.shape == (S, 7, K)
    for flags in M.flag_sets(K):
        res = M.solve(xbar, ubar, consts, r_des, Ks, opts, flags)
        for f in M.FIELDS:
            assert np.array_equal(res[f], parent[f"{name}.f{flags}.{f}"]), (name, flags, f)
