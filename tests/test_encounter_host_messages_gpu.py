"""A call the listed-pair entry points refuse is answered as it was before their host side was put on shared code
(csrc/encounter_host.hpp: one description of the list and its sides, one set of argument tests; DeviceArena::result, host_run): the
same return code and the same mpcx_last_error text, character for character, in the host-pointer and the _dev form -- and, where a
call has two defects, the same one reported.  tests/golden/encounter_host_messages.json holds the answers of the library built from
the commit before that change; tests/golden/make_encounter_host_messages.py lists the cases and wrote it.  Every stored answer is
MPCX_E_BADARG, given before anything is enqueued: no case reaches a kernel."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_encounter_host_messages as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parent(golden_dir):
    with open(os.path.join(golden_dir, M.NAME)) as f:
        return json.load(f)


def test_every_entry_point_of_the_family_is_in_the_table(parent):
    assert sorted(parent) == sorted(M.CASES)
    assert all(rc == M.BADARG and msg for cases in parent.values() for forms in cases.values() for rc, msg in forms.values())


@pytest.mark.parametrize("name", list(M.CASES))
def test_refused_as_by_the_parent_build(parent, name):
    got = M.responses(name)
    assert {c: sorted(f) for c, f in got.items()} == {c: sorted(f) for c, f in parent[name].items()}
    for case, forms in got.items():
        for form, answer in forms.items():
            assert answer == parent[name][case][form], (name, case, form, answer, parent[name][case][form])
