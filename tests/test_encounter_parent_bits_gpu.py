"""The encounter kernels take their trajectory geometry (csrc/trajectory_device.hpp), the covariance chains their prologue and the
Gates row (csrc/covariance_device.hpp) and the refine loops and the Monte Carlo their flight set (encounter_host.hpp's FlightSet) from
shared functions.  That moves text, not arithmetic: every build must still give, byte for byte, what the library gave before.
tests/golden/encounter_parent_bits.npz holds inputs and results written by that older library
(tests/golden/make_encounter_parent_bits.py, which lists the cases and what each reaches): the ephemeris, both screens and the three
list calls behind them, both covariance chains, the five figures of a listed pair in both forms, the three refine loops and the joint
manoeuvre, and the Monte Carlo in both forms.  Compared are the integer views of every result (the sign of a zero and the payload of
a NaN count), or the SHA-256 of the larger ones."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_encounter_parent_bits as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parent(golden_dir):
    return np.load(os.path.join(golden_dir, M.NAME))


@pytest.mark.parametrize("case", M.CASES)
def test_bytes_of_the_parent_build(parent, case):
    res = M.results(case, M.inputs_of(parent, case))
    stored = {k.replace(".sha256", "").replace(".shape", "") for k in parent.files if k.startswith(f"{case}.out.")}
    assert stored == {f"{case}.out.{k}" for k in res}
    for k, a in res.items():
        assert M.differs(f"{case}.out.{k}", a, parent) is None, (case, k, M.differs(f"{case}.out.{k}", a, parent))
