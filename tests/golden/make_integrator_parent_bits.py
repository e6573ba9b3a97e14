#!/usr/bin/env python3
"""Bits of the two integrating kernels BEFORE propagate_kernel and discretize_kernel took their step-size control, dense output,
hold node, reciprocals and perturbation rules from shared functions (csrc/integrator_device.hpp, mpcx_device.hpp): inputs and
results of the project's own small cases, written by the library built from the commit before that change.
tests/test_integrator_parent_bits_gpu.py holds every later build to them byte for byte.

Needs an MI355X and the OLD library: build the parent commit in a checkout of its own and name its libmpcx.so in MPCX_LIB
(mpconstellation_amd/_ffi.py loads that file instead of the tree's own):

    MPCX_LIB=/path/to/parent/mpconstellation_amd/libmpcx.so python tests/golden/make_integrator_parent_bits.py [OUT.npz]

`check` as the only argument runs whatever library is loaded on the stored inputs and compares instead of writing.

The file's layout and helpers are make_encounter_parent_bits.py's: `<case>.in.<name>`, `<case>.out.<call>.<field>`, values, status
and nsteps arrays alike; a result above BIG bytes (1 KiB here: there are some 500 arrays) is held by its SHA-256 and shape.

case        entry points and what they reach
roll00-15   every case of rollout_cases.device_cases() through propagate_batch with u_out: max_step 1 and 0.05, rejected attempts,
            1 to 40 output points, a ragged launch, every law and flag set
rollinf, roll2, rollnan
            the mixed waves at max_step = inf and 2, and at 1 with a NaN quad (MPCX_ST_STEP after some 460 attempts)
clipped     max_step = 1e-3, where only the rollout's two shortcuts run: S = 17 (a wave of 16 quads and one quad), n_eval = 5 with
            u_out, each of the four laws under each of the six flag sets of MPCX_PROP_FLAGS; one ragged sequence launch with a
            row of one output point and a row whose Ku is out of range (MPCX_ST_BADK)
resample    mpcx_resample_sequence_dev on a ragged table: foh3, tau == 1 at every row's last node, a row of one node
disc.<case> discretize_cases' case in every mode it lists at max_step = 1, and in rk45, rk23, uni5 and rk23+uni7 at 1e-2 (the
            benchmark's regime: no pow), in the stage layout; where the case is not ragged the reference layout as well
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)
from make_encounter_parent_bits import arrays_of, differs, inputs_of, stored        # noqa: E402

NAME = "integrator_parent_bits.npz"
BIG = 1024
ST_STEP, ST_BADK = 2, 9
LAW_ARRAYS = ("table", "end_tau", "constant", "tangential")


# ---------------------------------------------------------------- rollouts
def roll_cases():
    """name -> (case of rollout_cases, max_step or None for its own, NaN quad)"""
    import rollout_cases as R
    out = {f"roll{i:02d}": (c, None, False) for i, c in enumerate(R.device_cases())}
    out.update(rollinf=(R.mixed_waves(), float("inf"), False), roll2=(R.mixed_waves(), 2.0, False), rollnan=(R.mixed_waves(), None, True))
    return out


def build_roll(name):
    import rollout_cases as R
    c, _, nan = roll_cases()[name]
    w = dict(y0=c["y0"].copy(), tf=c["tf"], const=c["const"], n_eval=np.asarray(c["n_eval"]))
    if nan:
        w["y0"][R.BAD_SAT, R.BAD_COMPONENT] = np.nan
    w.update({k: c[k] for k in LAW_ARRAYS if k in c})
    return w


def device_law(law, w):
    from mpconstellation_amd import _ffi
    return {"zero": lambda: (_ffi.CTRL_ZERO, None, 0, None), "constant": lambda: (_ffi.CTRL_CONSTANT, w["constant"], 0, None),
            "tangential": lambda: (_ffi.CTRL_TANGENTIAL, w["tangential"], 0, None),
            "sequence": lambda: (_ffi.CTRL_SEQUENCE, w["table"], w["table"].shape[2], w["end_tau"])}[law]()


def run_roll(name, w):
    import rollout_cases as R
    from mpconstellation_amd.simulator import propagate_batch
    c, max_step, nan = roll_cases()[name]
    n = w["n_eval"] if w["n_eval"].ndim else int(w["n_eval"])
    y, st, ns, u = propagate_batch(w["y0"], w["tf"], w["const"], device_law(c["law"], w), n, include_drag=bool(c["flags"] & R.DRAG),
                                   include_J2=bool(c["flags"] & R.J2), max_step=c["max_step"] if max_step is None else max_step, thrust=True,
                                   atmosphere=c["atmosphere"])
    assert st.tolist() == [ST_STEP if nan and s == R.BAD_SAT else 0 for s in range(len(st))], st
    return dict(flight=(y, st, ns, u))


# ---------------------------------------------------------------- rollouts at max_step = 1e-3
CLIPPED_S, CLIPPED_N, CLIPPED_KU = 17, 5, 12
CLIPPED_FLAGS = {"none": (False, False, False), "drag": (True, False, False), "j2": (False, True, False), "drag+j2": (True, True, False),
                 "drag+atmo": (True, False, True), "drag+j2+atmo": (True, True, True)}


def build_clipped():
    """the low orbits of drag_cases.rollout_case (the only ones its atmosphere is anything on), S = 17 of them a part in 1e3 apart"""
    import drag_cases as D
    c = D.rollout_case()
    rng = np.random.default_rng(17)
    idx = np.arange(CLIPPED_S) % 3
    n_evals = np.full(CLIPPED_S, CLIPPED_N, dtype=np.int32); n_evals[3] = 1
    Kus = np.full(CLIPPED_S, CLIPPED_KU, dtype=np.int32); Kus[16] = CLIPPED_KU + 1; Kus[9] = 7
    return dict(y0=c["y0"][idx] * (1.0 + 1e-3 * rng.standard_normal((CLIPPED_S, 7))), tf=np.array([0.5, 0.25, 0.4])[idx], const=c["const"][idx],
                constant=rng.normal(size=(CLIPPED_S, 3)) * 0.1, tangential=rng.uniform(0.1, 0.5, CLIPPED_S), table=rng.normal(size=(CLIPPED_S, 3, CLIPPED_KU)) * 0.1,
                end_tau=np.array([1.0, 0.6, 1.0])[idx], n_evals=n_evals, Kus=Kus)


def run_clipped(w):
    import drag_cases as D
    from mpconstellation_amd.simulator import propagate_batch
    out = {}
    for law in D.LAWS:
        for tag, (drag, j2, atmo) in CLIPPED_FLAGS.items():
            r = propagate_batch(w["y0"], w["tf"], w["const"], device_law(law, w), CLIPPED_N, include_drag=drag, include_J2=j2, max_step=1e-3, thrust=True,
                                atmosphere=D.models()["general"] if atmo else None)
            assert (r[1] == 0).all() and (r[2] >= 250).all(), (law, tag, r[1], r[2])
            out[f"{law}.{tag}"] = r
    r = propagate_batch(w["y0"], w["tf"], w["const"], device_law("sequence", w), w["n_evals"], include_drag=True, include_J2=True, max_step=1e-3, thrust=True,
                        Kus=w["Kus"])
    assert r[1].tolist() == [0] * 16 + [ST_BADK], r[1]
    out["ragged"] = r
    return out


# ---------------------------------------------------------------- the hold alone
def build_resample():
    rng = np.random.default_rng(3)
    return dict(u=rng.standard_normal((7, 3, 9)), Kus=np.array([2, 9, 5, 3, 9, 7, 4], dtype=np.int32), ns=np.array([12, 1, 7, 12, 2, 9, 5], dtype=np.int32))


def run_resample(w):
    import torch
    from mpconstellation_amd import _ffi
    S, _, Ku = w["u"].shape
    n = int(w["ns"].max())
    dev = torch.device("cuda", 0)
    d_u = torch.tensor(w["u"], dtype=torch.float64, device=dev); d_out = torch.full((S, 3, n), float("nan"), dtype=torch.float64, device=dev)
    d_k = torch.tensor(w["Kus"], device=dev); d_n = torch.tensor(w["ns"], device=dev); d_st = torch.full((S,), -1, dtype=torch.int32, device=dev)
    lib, ctx = _ffi.load(), _ffi.context(0)
    p = lambda t: C.c_void_p(t.data_ptr())
    _ffi.check(lib.mpcx_resample_sequence_dev(ctx, S, Ku, p(d_k), p(d_u), n, p(d_n), p(d_out), p(d_st), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
               ctx, "resample")
    torch.cuda.synchronize()
    out, st = d_out.cpu().numpy(), d_st.cpu().numpy()
    assert (st == 0).all()
    for s in range(S):
        if w["ns"][s] > 1:
            assert np.array_equal(out[s, :, w["ns"][s] - 1], w["u"][s, :, w["Kus"][s] - 1])           # tau == 1: the last column in use
    return dict(resample=(out, st))


# ---------------------------------------------------------------- discretiser
DISC = ("plain", "plain+j2", "drag-fixed", "drag-general", "drag-general-k4", "one")
CLIPPED_MODES = ("rk45", "rk23", "uni5", "rk23+uni7")


def build_disc(name):
    import discretize_cases as DC
    c = DC.case(name)
    return {k: c[k] for k in ("x", "u", "tf", "const", "Ks")}


def run_disc(name, w):
    import dev_solve
    import discretize_cases as DC
    from mpconstellation_amd import _ffi
    meta = DC.case(name)                                 # (flags, model, modes: the arrays are the stored ones)
    atm = DC.atmosphere(meta)
    drag, j2 = bool(meta["flags"] & DC.DRAG), bool(meta["flags"] & DC.J2)
    S, _, K = w["x"].shape
    ragged = bool((w["Ks"] != K).any())
    out = {}
    for max_step, modes in ((DC.MAX_STEP, meta["modes"]), (DC.CLIPPED_STEP, CLIPPED_MODES)):
        for mode in modes:
            fl, uni = DC.MODES[mode]
            flags = _ffi.discretize_flags(drag, j2, uniform_steps=uni, rk23=bool(fl & DC.RK23), atmosphere=atm)
            ctx = _ffi.atmosphere_context(0, 0, atm if drag else None)
            stage, st = dev_solve.discretize_stages(w["x"], w["u"], w["tf"], w["const"], Ks=w["Ks"] if ragged else None, flags=flags, max_step=max_step)
            assert (st == 0).all(), (name, mode, max_step, st)
            key = f"{mode}.{max_step:g}"
            out[key + ".stage"] = (stage.cpu().numpy(), st)
            if not ragged:
                n = S * (K - 1)
                ref = [np.full((n, 7, 7), np.nan), np.full((n, 7, 3), np.nan), np.full((n, 7, 3), np.nan), np.full((S, 7, K - 1), np.nan),
                       np.full((S, 7, K - 1), np.nan), np.full(S, -1, dtype=np.int32)]
                _ffi.check(_ffi.load().mpcx_discretize_batch(ctx, S, K, w["u"].shape[2], _ffi.dptr(_ffi.as_f64(w["x"])), _ffi.dptr(_ffi.as_f64(w["u"])),
                                                             _ffi.dptr(_ffi.as_f64(w["tf"])), _ffi.dptr(_ffi.as_f64(w["const"])), flags, float(max_step),
                                                             *[_ffi.dptr(a) for a in ref[:5]], _ffi.iptr(ref[5])), ctx, "mpcx_discretize_batch")
                assert (ref[5] == 0).all()
                out[key + ".ref"] = tuple(ref)
    return out


def case_names():
    return list(roll_cases()) + ["clipped", "resample"] + [f"disc.{n}" for n in DISC]


def build(case):
    if case.startswith("roll"):
        return build_roll(case)
    if case.startswith("disc."):
        return build_disc(case[5:])
    return {"clipped": build_clipped, "resample": build_resample}[case]()


def results(case, w):
    """{`<call>.<field>`: array} of the loaded library on the case's inputs"""
    if case.startswith("roll"):
        return arrays_of(run_roll(case, w))
    if case.startswith("disc."):
        return arrays_of(run_disc(case[5:], w))
    return arrays_of({"clipped": run_clipped, "resample": run_resample}[case](w))


def main():
    import torch
    torch.cuda.is_available()        # (the wheel's HIP runtime has to be the first one initialised in the process: tests/conftest.py)
    check = sys.argv[1:] == ["check"]
    path = os.path.join(HERE, NAME) if check or not sys.argv[1:] else sys.argv[1]
    old = np.load(path) if check else None
    out, bad = {}, 0
    for case in case_names():
        w = inputs_of(old, case) if check else build(case)
        res = results(case, w)
        print(f"{case:20s}: {len(w)} inputs of {sum(a.nbytes for a in w.values())} bytes, {len(res)} results of {sum(a.nbytes for a in res.values())} bytes", flush=True)
        if check:
            for k, a in res.items():
                what = differs(f"{case}.out.{k}", a, old)
                if what:
                    bad += 1
                    print(f"    {k}: {what}")
            want = {k.replace(".sha256", "").replace(".shape", "") for k in old.files if k.startswith(f"{case}.out.")}
            missing = want - {f"{case}.out.{k}" for k in res}
            bad += len(missing)
            for k in sorted(missing):
                print(f"    {k}: stored, not returned")
        else:
            out.update({f"{case}.in.{k}": np.asarray(a) for k, a in w.items()})
            for k, a in res.items():
                out.update(stored(f"{case}.out.{k}", a, BIG))
    if check:
        print("identical" if not bad else f"{bad} arrays differ")
        return 1 if bad else 0
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
