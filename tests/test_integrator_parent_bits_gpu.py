"""propagate_kernel and discretize_kernel take scipy's step-size control, the dense output, the hold's node, the Newton reciprocals
and the drag and J2 rules from shared functions (csrc/integrator_device.hpp, mpcx_device.hpp).  That moves text, not arithmetic:
every build must still give, byte for byte, what the library gave before.  tests/golden/integrator_parent_bits.npz holds inputs and
results written by that older library (tests/golden/make_integrator_parent_bits.py, which lists the cases and what each reaches):
every rollout of tests/rollout_cases.py with its thrust output, the rollout at max_step = 1e-3 under every law and flag set, the
hold on a ragged table, and every case of tests/discretize_cases.py in each of its modes at max_step = 1 and 1e-2 in both layouts.
Compared are the integer views of every result -- values, status and step counts; the sign of a zero and the payload of a NaN
count -- or the SHA-256 of the larger ones."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_integrator_parent_bits as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parent(golden_dir):
    return np.load(os.path.join(golden_dir, M.NAME))


@pytest.mark.parametrize("case", M.case_names())
def test_bytes_of_the_parent_build(parent, case):
    res = M.results(case, M.inputs_of(parent, case))
    stored = {k.replace(".sha256", "").replace(".shape", "") for k in parent.files if k.startswith(f"{case}.out.")}
    assert stored == {f"{case}.out.{k}" for k in res}
    for k, a in res.items():
        assert M.differs(f"{case}.out.{k}", a, parent) is None, (case, k, M.differs(f"{case}.out.{k}", a, parent))
