"""The list of tests/solve_active_cases.py held to its own criteria on the CPU oracle (oracle/nlp_ipm.py), so that nobody who edits
it later can weaken it silently.  A case stays in the list only if

* the oracle ends it with status 0 and without a regularised iteration;
* every family it declares is active by the census (slack <= 1e-6, multiplier >= 1e-2; |NU| >= 1e-3);
* it is no knife edge: the dense mode (LAPACK on the un-condensed system) and the solve on u_bar (1 + 2^-40) take the same
  number of iterations and end within 1e-9 of the plain solve;
* its last convergence decision is not marginal: the final scaled error is <= tol / 2, or the iterate before was still at
  >= 2 tol -- a device that rounds otherwise takes the same number of iterations;
* (K >= 24) the partitioned algebra the time-parallel kernel implements (tests/tools/partitioned_riccati.py, four segments) ends
  with status 0 after the same number of iterations.  Its distance delta_part from the sequential solve decides whether the
  device's time-parallel kernel is held to 1e-9 or to the solver tolerance (solve_active_cases.tp_tight).

... and the list as a whole names every family, the stage families at K = 30 and at K = 60.

Measured when the list was made: delta_part <= 1e-12 on ten of the fifteen cases with K >= 24, <= 1e-10 on all; dense and
perturbed solves within 1e-10 of the plain one.  Left out on purpose: the exact variant under a thrust
limit or a tight mass floor (the structured and the dense mode end at different local minima) and w_nu = 0.01 (the dense mode
ends "acceptable")."""
import numpy as np
import pytest

import solve_active_cases as A

N = A.N
TOL = 1e-8               # N.solve's tol
KNIFE = 1e-9


@pytest.mark.parametrize("cid", A.IDS)
def test_case_meets_the_criteria(cid):
    case = A.BY_ID[cid]
    P, ref, cen = A.reference(cid)
    assert ref["status"] == 0 and ref["n_regularised"] == 0
    for family in case["declares"]:
        assert cen[family], (family, {f: sorted(v) for f, v in cen.items() if v})
    dense = N.solve(P, dense=True)
    nudged = N.solve(A.problem(case, u_scale=1.0 + 2.0 ** -40))
    for other in (dense, nudged):
        assert other["status"] == 0 and other["iters"] == ref["iters"]
        assert A.delta(other, ref) <= KNIFE
    if ref["kkt"] > TOL / 2:
        before = N.solve(P, max_iter=ref["iters"] - 1)
        assert before["iters"] == ref["iters"] - 1 and before["kkt"] >= 2 * TOL, (ref["kkt"], before["kkt"])


def test_the_list_covers_every_family():
    declared = lambda pick: set(f for c in A.CASES if pick(c) for f in c["declares"])
    assert declared(lambda c: True) == set(A.FAMILIES)
    for K in (30, 60):
        assert set(A.STAGE_FAMILIES) <= declared(lambda c: c["K"] == K), K
    assert set(c["variant"] for c in A.CASES) == {"exact", "linvt"}
    assert [c["id"] for c in A.CASES if c["K"] < A.TP_MIN_K] and len(A.TP_IDS) >= 12


@pytest.mark.parametrize("cid", A.TP_IDS)
def test_partitioned_algebra_follows_the_same_path(cid):
    _, ref, _ = A.reference(cid)
    part, delta_part = A.partitioned(cid)
    print(f"{cid}: iterations {part['iters']} / sequential {ref['iters']}, delta_part {delta_part:.2e}, tp_tight {A.tp_tight(cid)}")
    assert part["status"] == 0 and part["iters"] == ref["iters"]
    assert np.isfinite(delta_part) and A.tp_tight(cid) == (delta_part <= A.TP_TIGHT)
    assert N.riccati_channel is __import__("partitioned_riccati").SEQ_CHANNEL            # the patch was taken out again
