"""The window manoeuvre flown and corrected (avoidance_window_refine_reference.py, the restatement of include/mpcx.h:
mpcx_avoidance_window_refine) without a GPU: the loop on the host tests' slow pair under the CPU oracle's flight and discretisation,
tracked and untracked, and the wrapper's argument checks, empty list, result columns and exports.  The measured figures quoted below
are in profiles/avoidance_window_refine.txt."""
import functools

import numpy as np
import pytest

import avoidance_reference as AR
import avoidance_window_reference as AW
import avoidance_window_refine_reference as RF
from test_avoidance_window_host import slow_pair, HALF, PANELS, GOOD, CAT, U, N

ROUNDS = 2
GRID = 4 * (AR.SCENE["K"] - 1) + 1


@functools.lru_cache(maxsize=None)
def slow_pair_loop(tracked):
    """the restated loop on slow_pair(): a target two decades below Q0, two rounds.  Treat as read-only."""
    sc, t, rows, cat, pairs, stage = slow_pair()
    grads = AW.row_gradients(pairs, rows, HALF, PANELS, cat)
    target = 1e-2 * (grads[0]["start"] + grads[0]["entries"])
    track = (GRID, float(sc["span"][0]), float(sc["span"][1])) if tracked else None
    return target, RF.refine(pairs, rows, sc["U"][None], sc["consts"][None], target, HALF, PANELS, ROUNDS, cols=cat, track=track, stage0=stage,
                             max_step=AR.SCENE["disc_max_step"], prop_max_step=AR.SCENE["prop_max_step"])


def flown_gaps(res, target):
    """|ln(Q_flown / target)| of the flights 1 .. rounds + 1"""
    return np.abs(np.log(res["p_history"][1:, 0] / target))


@pytest.mark.parametrize("tracked", [True, False])
def test_loop_closes_the_linearisation_gap(tracked):
    """The issue's conditions on the restated loop.  Tracked, the first flight misses the target by at least 0.05 in ln P -- the gap the
    loop exists for; in both modes the last flight is at most 1e-2 of the first flight's miss; every solve after pass 1 needs at most 4
    evaluations.  Measured when written (profiles/avoidance_window_refine.txt): tracked 1.41e-1 -> 7.4e-4 -> 5.1e-7 with the event at
    -48.6 s then -49.8 s; untracked 1.6e-3 -> 5.6e-6 -> 2.9e-7."""
    target, res = slow_pair_loop(tracked)
    gaps = flown_gaps(res, target)
    sc, t = slow_pair()[:2]
    print(f"{'tracked' if tracked else 'untracked'}: target {target:.4e}, |ln(Q_flown / target)| per flight {[f'{g:.3e}' for g in gaps]}, "
          f"event at {[f'{x - t:+.2f}' for x in res['t_history'][:, 0]]} s, evaluations per solve {res['evals'][:, 0].astype(int).tolist()}, "
          f"rounds_done {res['rounds_done'].tolist()}, status {res['status'].tolist()}")
    assert res["status"].tolist() == [0] and res["rounds_done"].tolist() == [ROUNDS]
    assert res["p_history"][0, 0] == res["out"][0, AW.P0] and np.isfinite(res["p_history"]).all()
    if tracked:
        assert gaps[0] >= 0.05 and (res["t_history"][1:, 0] != t).all()
    else:
        assert (res["t_history"][:, 0] == t).all()
    assert gaps[-1] <= 1e-2 * gaps[0]
    assert (res["evals"][2:, 0] <= 4).all() and (res["evals"][1:, 0] >= 1).all()
    # every solve's prediction is within tol of the target, and the total change keeps pass 0's shape of columns
    assert (np.abs(np.log(res["p_predicted"][:, 0] / target)) <= 1e-6).all()
    assert res["out"][0, AW.EVALS] == res["evals"][:, 0].sum() and res["out"][0, AW.P1] == res["p_predicted"][-1, 0]
    assert res["du"].shape == (1, 1, 3, AR.SCENE["K"]) and res["du"][0, 0].any() and res["Y_flown"].shape == (1, 1, 7, AR.SCENE["K"])


def test_rounds_zero_is_the_first_order_manoeuvre_flown_once():
    """rounds = 0: avoidance_window's answer, one flight, one figure; a solve that runs out of evaluations in pass 1 keeps pass 0's du,
    reports its status and repeats its flight"""
    sc, t, rows, cat, pairs, stage = slow_pair()
    target, full = slow_pair_loop(False)
    kw = dict(cols=cat, stage0=stage, max_step=AR.SCENE["disc_max_step"], prop_max_step=AR.SCENE["prop_max_step"])
    res = RF.refine(pairs, rows, sc["U"][None], sc["consts"][None], target, HALF, PANELS, 0, **kw)
    assert res["p_history"].shape == (2, 1) and res["p_history"][1, 0] == full["p_history"][1, 0] and res["rounds_done"].tolist() == [0]
    grads = AW.row_gradients(pairs, rows, HALF, PANELS, cat)
    sens, Es, st = AW.window_sensitivity(grads, rows, stage, "i", cat)
    out, du, status, _ = AW.avoidance_window(grads, sens, Es, st, rows, stage, target, 1e-6, 40, PANELS, "i", cat)
    assert np.array_equal(res["du"], du) and np.array_equal(res["out"], out)
    short = RF.refine(pairs, rows, sc["U"][None], sc["consts"][None], target, HALF, PANELS, 1, tol=1e-12, max_eval=[40, 1], **kw)
    assert short["status"].tolist() in ([RF.ST_MAXITER], [RF.ST_INFEASIBLE]) and short["rounds_done"].tolist() == [0]
    assert np.array_equal(short["du"], RF.refine(pairs, rows, sc["U"][None], sc["consts"][None], target, HALF, PANELS, 0, tol=1e-12, **kw)["du"])
    assert short["p_history"][1, 0] == short["p_history"][2, 0]
    below = RF.refine(pairs, rows, sc["U"][None], sc["consts"][None], 0.5, HALF, PANELS, 1, **kw)
    assert below["status"].tolist() == [0] and not below["du"].any() and below["rounds_done"].tolist() == [-1]
    assert (below["p_history"][:, 0] == below["out"][0, AW.P0]).all() and np.isnan(below["p_predicted"]).all()


# ---------------------------------------------------------------- the wrapper without a device
def test_wrapper_argument_checks():
    from mpconstellation_amd import conjunction as cj
    base = dict(target_p=1e-4, **GOOD)
    for kw in (dict(pairs=np.zeros((1, 3))), dict(P=None), dict(who="k"), dict(cat=CAT, who="j"), dict(half_window=None), dict(panels=0),
               dict(target_p=0.0), dict(target_p=1.0), dict(target_p=np.nan), dict(tol=0.0), dict(max_eval=0), dict(max_eval=2.5),
               dict(rounds=-1), dict(rounds=1.5), dict(prop_max_step=0.0), dict(track=(1, 0.0, 1.0)), dict(track=(5, 1.0, 1.0)),
               dict(track=(5, 0.0)), dict(track=(5, 0.0, 1.0), max_shift=np.nan), dict(recov=True, q=[1.0, 2.0, 3.0]), dict(recov=True, q=-1.0),
               dict(max_step=0.0)):
        with pytest.raises(ValueError):
            cj.avoidance_window_refine(**{**base, **kw})
    with pytest.raises(ValueError, match="rounds"):
        cj.avoidance_window_refine(**{**base, "rounds": -2})
    with pytest.raises(ValueError, match="track"):
        cj.avoidance_window_refine(**{**base, "track": 7})


def test_the_empty_list_makes_no_library_call(monkeypatch):
    from mpconstellation_amd import conjunction as cj, _ffi

    def no_call(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_ffi, "call", no_call)
    monkeypatch.setattr(_ffi, "context", no_call)
    monkeypatch.setattr(_ffi, "atmosphere_context", no_call)
    for kw in (dict(), dict(cat=CAT), dict(devices=[0, 0]), dict(who="both", recov=True, q=1e-8), dict(track=(9, 0.0, 1.0), rounds=0)):
        NS = 1 if "cat" in kw else 2
        r = cj.avoidance_window_refine(target_p=1e-4, return_sensitivities=True, **{**GOOD, "pairs": np.zeros((0, 4)), **kw})
        rounds = kw.get("rounds", 2)
        assert isinstance(r, cj.AvoidanceWindowRefineResult) and isinstance(r, cj.AvoidanceWindowResult)
        assert r.du.shape == r.sens.shape == (0, NS, 3, N) and r.Y_flown.shape == (0, NS, 7, N) and r.p0.shape == r.evals.shape == (0,)
        assert r.p_history.shape == r.t_history.shape == (rounds + 2, 0) and r.p_predicted.shape == (rounds + 1, 0)
        assert r.rounds_done.shape == (0,) and r.rounds_done.dtype == np.int32 and r.status.dtype == np.int32
        assert (r.P_flown is None) == ("recov" not in kw) and (r.P_flown is None or r.P_flown.shape == (0, NS, N, 6, 6))
    with pytest.raises(AssertionError, match="the library was called"):
        cj.avoidance_window_refine(target_p=1e-4, **GOOD)


def test_result_columns_and_apply(monkeypatch):
    """the wrapper hands the library the window call's arguments, then target_p, tol, max_eval, prop_max_step, rounds, the grid,
    max_shift, recov and q; maps the columns by name; apply adds a row's total du to its satellites"""
    from mpconstellation_amd import conjunction as cj, _ffi
    seen = {}

    def fake_call(name, ctx, n, *args):
        tail = args[-21:]
        seen.update(name=name, n=n, target=tail[0], tol=tail[1], max_eval=tail[2], prop_max_step=tail[3], rounds=tail[4], grid=tail[5:9],
                    recov=tail[9], q=bool(tail[10]), sens=bool(tail[13]), P_flown=bool(tail[17]))
        out = np.ctypeslib.as_array(tail[11], shape=(n * _ffi.NAW,)).reshape(n, _ffi.NAW)
        out[:] = np.arange(_ffi.NAW)[None, :] + 10.0 * np.arange(n)[:, None]
        np.ctypeslib.as_array(tail[12], shape=(n * 2 * 3 * N,))[:] = 1.0
        np.ctypeslib.as_array(tail[15], shape=(n,))[:] = 2
        np.ctypeslib.as_array(tail[18], shape=(4 * n,))[:] = np.arange(4 * n)            # hist_p [rounds + 2][n]
    monkeypatch.setattr(_ffi, "call", fake_call)
    monkeypatch.setattr(_ffi, "atmosphere_context", lambda *a: None)
    pairs = np.array([[0.0, 1.0, 50.0, 0.25], [1.0, 0.0, 60.0, 0.5], [0.0, 1.0, 70.0, 0.75]])
    r = cj.avoidance_window_refine(target_p=1e-3, **{**GOOD, "pairs": pairs, "who": "both", "tol": 1e-4, "max_eval": 7, "rounds": 2,
                                                    "track": (9, 0.0, 1.0), "max_shift": 5.0, "recov": True, "q": 1e-8, "prop_max_step": 2e-3})
    assert seen == dict(name="mpcx_avoidance_window_refine", n=3, target=1e-3, tol=1e-4, max_eval=7, prop_max_step=2e-3, rounds=2,
                        grid=(9, 0.0, 1.0, 5.0), recov=1, q=True, sens=False, P_flown=True)
    assert r.p0.tolist() == [0.0, 10.0, 20.0] and r.p1.tolist() == [1.0, 11.0, 21.0] and r.alpha.tolist() == [2.0, 12.0, 22.0]
    assert r.dq_linear.tolist() == [3.0, 13.0, 23.0] and r.evals.tolist() == [8.0, 18.0, 28.0] and r.rounds_done.tolist() == [2, 2, 2]
    assert r.p_history.shape == (4, 3) and r.p_history[1].tolist() == [3.0, 4.0, 5.0] and r.P_flown.shape == (3, 2, N, 6, 6)
    U2 = r.apply(U, 1)
    assert U2.shape == U.shape and (U2 == 1.0).all() and not U.any()
    r.status[2] = 5
    with pytest.raises(ValueError, match="no manoeuvre"):
        r.apply(U, 2)
    cj.avoidance_window_refine(target_p=1e-3, **{**GOOD, "pairs": pairs, "recov": True, "return_covariances": False})
    assert seen["grid"] == (0, 0.0, 0.0, 0.0) and seen["P_flown"] is False and seen["q"] is False and seen["rounds"] == 2


def test_exports():
    import mpconstellation_amd as pkg
    from mpconstellation_amd import _ffi
    names = {"mpcx_avoidance_window_refine", "mpcx_avoidance_window_refine_dev", "mpcx_avoidance_window_refine_workspace_bytes"}
    assert names <= set(_ffi.exported_symbols())
    assert {"avoidance_window_refine", "AvoidanceWindowRefineResult"} <= set(pkg.__all__) and callable(pkg.avoidance_window_refine)
    assert callable(pkg.ConstellationMPC.avoidance_window_refine)


def test_constellation_avoidance_window_refine_needs_a_plan():
    from test_conjunction_host import hand_made_mpc
    mpc, _ = hand_made_mpc()
    with pytest.raises(ValueError, match="no plan"):
        mpc.avoidance_window_refine(1000.0, np.eye(6), 5.0, 60.0, 1e-6)
