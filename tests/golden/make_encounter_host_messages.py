#!/usr/bin/env python3
"""What the listed-pair entry points answer to a call they refuse -- return code and mpcx_last_error text -- BEFORE their host side
took its description of the list and its sides, its argument tests, its uploads, its results and its tail from shared code
(csrc/encounter_host.hpp, DeviceArena::result, host_run), written by the library built from the commit before that change.
tests/test_encounter_host_messages_gpu.py holds every later build to them character for character.

Needs an MI355X and the OLD library, named in MPCX_LIB as tests/golden/make_encounter_parent_bits.py describes:

    MPCX_LIB=/path/to/parent/mpconstellation_amd/libmpcx.so python tests/golden/make_encounter_host_messages.py [OUT.json]

`check` as the only argument asks whatever library is loaded and compares instead of writing.

Every case starts from one valid small call of its entry point (tests/encounter_abi.py: BASE) and applies the defects of its name: one
defect, or two -- one of the tests every call shares, one of the call's own -- which pins the order of the tests.  A case is asked of
the host-pointer form and of the _dev form (device tensors, a workspace of the right size); `workspace` cases of the _dev form alone,
`mover` cases of the host form alone (only there the library reads the array).  Only calls that the library refuses with
MPCX_E_BADARG before it enqueues anything belong here: writing asserts rc == -2 for every one of them, and the valid call's rc == 0."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))

NAME = "encounter_host_messages.json"
BADARG = -2
INF = float("inf")
UNKNOWN_FLAG = 1 << 20
BAD_MOVER = np.array([0, 2, 0], dtype=np.int32)


def null(*names):
    return [{k: None} for k in names]


# the defects of the tests the calls share, by what an entry point has
SIZES = [dict(n=0), dict(K=1), dict(mu=0.0)]
CATALOGUE = [dict(D=0), dict(cat_units=None)]
MODEL = [dict(flags=UNKNOWN_FLAG), dict(max_step=0.0)]
TARGET = [dict(target=0.0), dict(target=INF)]
WHO = [dict(who=3), dict(who=1)]
GEOMETRY_IN = ("pairs", "Y", "units", "span")
PLAN_IN = GEOMETRY_IN + ("U", "consts")
PROBABILITY = SIZES + CATALOGUE + null(*GEOMETRY_IN, "P", "radius", "cat_P", "cat_radius")
WINDOW = SIZES + CATALOGUE + MODEL + WHO + null(*PLAN_IN, "P", "radius", "half_window", "cat_P", "cat_radius") + [dict(panels=0)]
JOINT = (SIZES + CATALOGUE + MODEL + TARGET + null(*PLAN_IN, "du", "sat_out", "row_out", "sat_status", "row_status", "cat_P")
         + [dict(tol=0.0), dict(max_iter=0), dict(mover=BAD_MOVER), dict(workspace=None), dict(tol=0.0, K=1), dict(max_iter=0, target=0.0)])
REFINE = JOINT + null("Y_out", "pairs_out", "hist_d0", "hist_tca", "hist_term", "rounds_done") + [dict(rounds=-1), dict(M=1), dict(prop_max_step=0.0),
                                                                                                  dict(rounds=-1, tol=0.0)]
LIST = [dict(S=0), dict(M=1), dict(T1=0.0)] + null("pairs", "eph", "cat", "status")
COVARIANCE = [dict(S=0), dict(K=1)] + MODEL + null("X", "units", "span", "consts", "P0", "P", "status") + [dict(workspace=None), dict(K=1, X=None)]

CASES = {
    "mpcx_collision_probability": PROBABILITY + null("out", "status") + [dict(n=0, out=None), dict(pairs=None, D=0)],
    "mpcx_collision_probability_window": PROBABILITY + null("half_window", "out", "status") + [dict(panels=0), dict(panels=0, pairs=None),
                                                                                                dict(panels=0, mu=0.0)],
    "mpcx_encounter_window": PROBABILITY + null("max_half", "out", "flags", "status") + [dict(levels=0), dict(nsigma=0.0), dict(levels=0, pairs=None),
                                                                                          dict(levels=0, mu=0.0), dict(nsigma=INF, levels=0)],
    "mpcx_collision_window_sensitivity": WINDOW + null("out", "sens", "status") + [dict(workspace=None), dict(who=3, cat_P=None), dict(who=3, n=0),
                                                                                    dict(panels=0, pairs=None), dict(who=3, panels=0)],
    "mpcx_avoidance_window": WINDOW + null("out", "du", "status") + [dict(target_p=0.0), dict(target_p=INF), dict(target_p=1.0), dict(tol=0.0),
                                                                      dict(max_eval=0), dict(workspace=None), dict(tol=0.0, who=3),
                                                                      dict(max_eval=0, K=1), dict(target_p=1.0, panels=0)],
    "mpcx_avoidance_window_refine": WINDOW + null("out", "du", "status", "rounds_done", "Y_out", "hist_p", "hist_t", "hist_pred")
    + [dict(target_p=0.0), dict(tol=0.0), dict(max_eval=0), dict(workspace=None), dict(prop_max_step=0.0), dict(rounds=-1), dict(M=1), dict(recov=2),
       dict(M=1, max_eval=0), dict(recov=2, mu=0.0)],
    "mpcx_collision_probability_mc": [dict(n=0), dict(K=1), dict(D=0), dict(cat_units=None), dict(cat_radius=None), dict(cat_consts=None),
                                      dict(flags=UNKNOWN_FLAG), dict(prop_max_step=0.0), dict(scan=0), dict(n_samples=0), dict(max_flights=-1),
                                      dict(workspace=None), dict(scan=0, n=0), dict(n_samples=0, pairs=None), dict(max_flights=-1, D=0)]
    + null(*GEOMETRY_IN, "consts", "P0", "radius", "half_window", "counts", "out", "status"),
    "mpcx_avoidance": SIZES + CATALOGUE + MODEL + TARGET + WHO + null(*PLAN_IN, "out", "du", "status", "cat_P")
    + [dict(workspace=None), dict(who=3, target=0.0), dict(who=3, pairs=None), dict(who=1, cat_P=None)],
    "mpcx_avoidance_joint": JOINT + [dict(sat0=3), dict(sat0=-1), dict(nsat=0), dict(sat0=3, flags=UNKNOWN_FLAG), dict(mover=BAD_MOVER, sat0=3)],
    "mpcx_avoidance_refine": REFINE,
    "mpcx_avoidance_refine_tracked": REFINE + [dict(max_shift=float("nan"))],
    "mpcx_covariance_batch": COVARIANCE,
    "mpcx_covariance_thrust_batch": COVARIANCE + null("U", "exec"),
    "mpcx_conjunction_pairs": LIST + null("out") + [dict(n=0), dict(n=0, M=1)],
    "mpcx_conjunction_events": LIST + null("events", "info", "count") + [dict(max_events=0), dict(threshold=float("nan")), dict(max_events=0, S=0)],
    "mpcx_conjunction_track": LIST + null("out") + [dict(max_shift=float("nan")), dict(max_shift=float("nan"), S=0)],
}


def label(defect):
    return ", ".join(f"{k}={'NULL' if v is None else 'bad' if isinstance(v, np.ndarray) else v}" for k, v in defect.items())


def responses(name):
    """{case: {form: [rc, message]}} of the loaded library for every case of entry point `name`"""
    import encounter_abi as A
    base = A.base_call(name)
    dev = A.on_device(base)
    wsb = A.workspace_bytes(name, base)
    if wsb:
        import torch
        dev["workspace"] = torch.zeros(wsb // 8 + 1, dtype=torch.float64, device="cuda:0")
    out = {}
    for defect in CASES[name]:
        forms = {}
        if "workspace" not in defect:
            forms["host"] = [A.call_host(name, dict(base, **defect)), A.last_error()]
        if "mover" not in defect and ("workspace" not in defect or wsb):
            forms["dev"] = [A.call_dev(name, dict(dev, **defect)), A.last_error()]
        assert forms and label(defect) not in out, (name, defect)
        out[label(defect)] = forms
    return out


def base_is_valid(name):
    import encounter_abi as A
    rc = A.call_host(name, A.base_call(name))
    return rc == 0 or print(f"{name}: the valid call returns {rc}: {A.last_error()}")


def main():
    import torch                                                         # (the _dev forms' buffers; its HIP runtime has to be the first
    torch.cuda.init()                                                    #  one initialised in the process: tests/conftest.py)
    check = sys.argv[1:] == ["check"]
    path = os.path.join(HERE, NAME) if check or not sys.argv[1:] else sys.argv[1]
    old = json.load(open(path)) if check else None
    table, bad = {}, 0
    for name in CASES:
        if not check and not base_is_valid(name):
            bad += 1
            continue
        table[name] = responses(name)
        print(f"{name:40s}: {len(table[name])} cases")
        for case, forms in table[name].items():
            for form, (rc, msg) in forms.items():
                if check and old[name][case][form] != [rc, msg]:
                    bad += 1
                    print(f"    {case} ({form}): {rc} {msg!r}, stored {old[name][case][form]}")
                if not check and rc != BADARG:
                    bad += 1
                    print(f"    {case} ({form}): not refused: {rc} {msg!r}")
        if check and {c: sorted(f) for c, f in table[name].items()} != {c: sorted(f) for c, f in old[name].items()}:
            bad += 1
            print("    the stored cases are not these")
    if check:
        print("identical" if not bad else f"{bad} answers differ")
        return 1 if bad else 0
    if bad:
        print(f"{bad} cases are not refusals: nothing written")
        return 1
    with open(path, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{path}: {os.path.getsize(path)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
