"""The iterated avoidance on the device (mpcx_avoidance_refine in csrc/avoidance_joint.hip): with rounds = 0 the whole fly / re-screen /
linearise chain against the public calls it is made of, bit for bit; the KKT conditions of the last solve in float64 from what the
call returns; the three-encounter arc and the coupled scene against the restatement (avoidance_refine_reference.py) and inside the
host tests' bounds; the bits across forms and over a stale workspace; a satellite that fails at pass 0; ConstellationMPC; the C ABI.
Scenes come from test_avoidance_gpu.py, test_avoidance_joint_gpu.py and the host tests."""
import functools

import numpy as np
import pytest

import avoidance_joint_reference as J
import avoidance_reference as AR
from dev_solve import dev, filled, same_bits, _p, _stream
from test_avoidance_gpu import scene, union_of, arc_on_device
from test_avoidance_joint_gpu import arc_instance
from test_avoidance_joint_host import three_encounters, TARGET, FLOWN_BOUND
from test_avoidance_refine_host import arc_loop, arc_grid, coupled_scene, coupled_loop, shortfall, LOOP_BOUND, ROUNDS

pytestmark = pytest.mark.gpu

TOL = 1e-10
PROP_MAX_STEP = 1e-3


def grid_of(K):
    """the re-screen's grid of test_avoidance_gpu.scene: inside every row's and every object's span"""
    return dict(M=4 * (K - 1) + 1, T0=-1.0, T1=2999.0)


def targets(K):
    return (1000.0, 6.0) if K >= 30 else (1.0e7, 1.0e5)               # (test_avoidance_joint_gpu.py: rows of few nodes interpolate badly)


def sides(sc, P, cat):
    Y, units, span, ns = sc["rows"]
    c = None
    if cat:
        cY, cunits, cspan, cns, cP = sc["cat"]
        c = (cY, cunits, cspan, cP, cns) if P else (cY, cunits, cspan, cns)
    return dict(Y=Y, U=sc["U"], units=units, span=span, consts=sc["consts"], ns=ns, P=sc["P"] if P else None, cat=c)


def refine(sc, target, rounds, P=False, cat=True, **kw):
    from mpconstellation_amd import avoidance_refine
    kw.setdefault("return_rows", True); kw.setdefault("return_terminal", True); kw.setdefault("return_rhs", True)
    return avoidance_refine(sc["pairs"], target, **sides(sc, P, cat), **grid_of(sc["rows"][0].shape[2]), rounds=rounds, prop_max_step=PROP_MAX_STEP, **kw)


def joint(sc, target, P=False, cat=True, **kw):
    from mpconstellation_amd import avoidance_joint
    kw.setdefault("return_rows", True); kw.setdefault("return_terminal", True)
    s = sides(sc, P, cat)
    for k in ("pairs", "Y", "U"):
        if k in kw:
            s[k] = kw.pop(k)
    return avoidance_joint(s.pop("pairs", sc["pairs"]), target, **s, **kw)


def bits(r):
    return (r.du.tobytes(), r.sat_out.tobytes(), r.row_out.tobytes(), r.status.tobytes(), r.row_status.tobytes(), r.Y_flown.tobytes(),
            r.pairs_flown.tobytes(), r.d0_history.tobytes(), r.tca_history.tobytes(), r.terminal_history.tobytes(), r.rounds_done.tobytes())


def free_limits(sc, target, P, cat, hold, share):
    """u_max: `share` of each satellite's largest |ubar + du| without a ball, inf where there is none"""
    free = joint(sc, target, P=P, cat=cat, hold_terminal=hold, return_rows=False, return_terminal=False)
    u_max = np.where(free.status == 0, share * free.umax, np.inf)
    u_max[free.n_rows == 0] = np.inf
    return u_max


# ---------------------------------------------------------------- rounds = 0: the chain through public calls
# ball: the share of each satellite's free peak thrust that u_max is set to, None: no ball
CHAIN = [("catalogue", 3, 30, 3, False, True, True, 0.9), ("catalogue", 3, 30, 3, True, False, True, None), ("catalogue", 2, 8, 3, True, False, False, None),
         ("all-pairs", 1, 8, 2, False, False, True, None), ("all-pairs", 2, 30, 1, False, True, False, 0.9)]


@pytest.mark.parametrize("form,S,K,D,ragged,P,hold,ball", CHAIN)
def test_rounds_zero_is_the_chain_of_public_calls(form, S, K, D, ragged, P, hold, ball):
    """rounds = 0: du, sat_out, row_out, rows, tsens and the statuses are avoidance_joint's bits; Y_flown is propagate_batch under the
    applied table for every satellite that flies and the given trajectory for the others; pairs_flown is screen_pairs on it;
    d0_history[1] is avoidance_joint(pairs_flown, Y_flown, U + du).d0 -- the whole fly / re-screen / linearise chain"""
    from mpconstellation_amd import propagate_batch, screen_pairs, _ffi
    sc = scene(S, K, D, ragged)
    cat = form == "catalogue"
    if not cat:
        sc = union_of(sc)
    target = targets(K)[1 if P else 0]
    Y, units, span, ns = sc["rows"]
    n_sat = Y.shape[0]
    assert n_sat <= 3 and len(sc["pairs"]) <= 4
    if K < 30:
        # rows of 8 nodes interpolate a circle so badly that the planted pairs are far apart: half as far again as the farthest is a
        # manoeuvre the satellite can fly
        assert not P
        target = 1.5 * float(joint(sc, target, cat=cat, hold_terminal=False, return_rows=False, return_terminal=False).d0.max())
    u_max = free_limits(sc, target, P, cat, hold, ball) if ball else None
    res = refine(sc, target, 0, P=P, cat=cat, hold_terminal=hold, u_max=u_max)
    ref = joint(sc, target, P=P, cat=cat, hold_terminal=hold, u_max=u_max)
    print(f"{form} S {n_sat} K {K} ragged {ragged} P {P} hold {hold} ball {ball}: statuses {ref.status.tolist()}, rows {ref.n_rows.tolist()}, "
          f"d0 {res.d0_history.tolist()}, terminal {res.terminal_history.tolist()}")
    for name in ("du", "sat_out", "row_out", "rows", "tsens", "row_status"):
        assert same_bits(getattr(res, name), getattr(ref, name)), name
    flies = (ref.status == 0) & (ref.n_rows > 0)
    assert flies.any() and res.rounds_done.tolist() == np.where(flies, 0, -1).tolist()
    assert same_bits(res.rhs_rows[flies[res.pairs[:, 0].astype(int)]], (target - ref.d0)[flies[res.pairs[:, 0].astype(int)]]) and not res.rhs_term.any()
    # the flight
    counts = np.full(n_sat, K, dtype=np.int32) if ns is None else ns
    Ut = np.where(flies[:, None, None], sc["U"] + np.where(flies[:, None, None], ref.du, 0.0), sc["U"])
    tf = (span[:, 1] - span[:, 0]) / units[:, 1]
    y, st, _ = propagate_batch(np.ascontiguousarray(Y[:, :, 0]), tf, sc["consts"], (_ffi.CTRL_SEQUENCE, Ut, K, 1.0), counts if ns is not None else K,
                               max_step=PROP_MAX_STEP, Kus=None if ns is None else counts)
    flown = flies & (st == 0)
    assert flown.any() and np.array_equal(res.status, np.where(flies & ~flown, st, ref.status))         # (a failed flight is reported and flies nothing)
    Yf = Y.copy()
    for s in np.flatnonzero(flown):
        Yf[s] = 0.0
        Yf[s, :, :y.shape[2]] = y[s]
    assert same_bits(res.Y_flown, Yf)
    term = np.array([np.abs(Yf[s, :6, counts[s] - 1] - Y[s, :6, counts[s] - 1]).max() if flown[s] else 0.0 for s in range(n_sat)])
    assert same_bits(res.terminal_history, np.stack([np.zeros(n_sat), term])) and (term[flown] > 0.0).all()
    # the re-screen
    g = grid_of(K)
    catkw = {}
    if cat:
        cY, cunits, cspan, cns, _ = sc["cat"]
        catkw = dict(cat_Y=cY, cat_units=cunits, cat_span=cspan, cat_ns=cns)
    again = screen_pairs(sc["pairs"], g["T0"], g["T1"], Y=Yf, units=units, span=span, ns=ns, M=g["M"], **catkw)[0]
    assert same_bits(res.pairs_flown, again)
    assert same_bits(res.tca_history, np.stack([sc["pairs"][:, 3], again[:, 3]]))
    # the rows of the flown state
    flown = joint(sc, target, P=P, cat=cat, hold_terminal=hold, u_max=u_max, pairs=again, Y=Yf, U=Ut, return_rows=False, return_terminal=False)
    assert same_bits(res.d0_history, np.stack([ref.d0, flown.d0]))


# ---------------------------------------------------------------- the KKT conditions of the last solve
def test_kkt_of_the_final_manoeuvre():
    """S 3, K 30, catalogue, covariances, hold, ball at 0.9 of the free peak, rounds = 2: for every satellite whose last solve was
    accepted, from du, lambda, rows, tsens, rhs_rows and rhs_term in float64 -- feasibility and complementarity of the rows as solved,
    the terminal rows, the ball around the GIVEN thrust, and stationarity du = proj(U + (A^T z) / D) - U with D from the trajectory the
    last solve linearised about (the Y_flown of the same call with one round less)"""
    S, K, D = 3, 30, 3
    sc = scene(S, K, D, False)
    target = targets(K)[1]
    u_max = free_limits(sc, target, True, True, True, 0.9)
    res = refine(sc, target, 2, P=True, hold_terminal=True, u_max=u_max)
    before = refine(sc, target, 1, P=True, hold_terminal=True, u_max=u_max, return_rows=False, return_terminal=False, return_rhs=False)
    Y, units, span, ns = sc["rows"]
    done = np.flatnonzero(res.rounds_done == 2)
    print(f"statuses {res.status.tolist()}, rounds_done {res.rounds_done.tolist()}, rows {res.n_rows.tolist()}, active {res.n_active.tolist()}, on the ball "
          f"{res.n_on_ball.tolist()}, iterations of the last solve {res.iters.tolist()}, d0 by pass {res.d0_history.tolist()}")
    assert len(done) >= 1 and (res.n_on_ball[done] >= 1).any()
    for s in done:
        mine = np.flatnonzero(sc["pairs"][:, 0] == s)
        Dm, _, _ = J.effort_weights(before.Y_flown, units, span, ns, s)
        du, ub = res.du[s], sc["U"][s]
        a, lam, b = res.rows[mine], res.lam[mine], res.rhs_rows[mine]
        slack = np.einsum("pcm,cm->p", a, du) - b
        assert (slack >= -10.0 * TOL * target).all() and (lam >= 0.0).all() and (slack[lam > 0.0] <= 10.0 * TOL * target).all(), (s, slack, lam)
        nrm = np.sqrt(((ub + du) ** 2).sum(axis=0))
        assert (nrm <= u_max[s] * (1.0 + 10.0 * TOL)).all() and res.umax[s] <= u_max[s] * (1.0 + 10.0 * TOL)
        T = res.tsens[s]
        assert np.abs(np.einsum("icm,cm->i", T, du) - res.rhs_term[s]).max() <= 10.0 * TOL and res.rhs_term[s].any()
        v = np.einsum("p,pcm->cm", lam, a)
        inside = nrm < u_max[s] * (1.0 - 1e-9)
        y = np.linalg.lstsq(T[:, :, inside].reshape(6, -1).T, (Dm * du - v)[:, inside].ravel(), rcond=None)[0]
        v = v + np.einsum("i,icm->cm", y, T)
        pp, _, out = J.project(ub + v / Dm, u_max[s])
        err = np.abs(pp - ub - du).max()
        assert err <= 10.0 * TOL * np.abs(du).max(), (s, err, np.abs(du).max())
        assert int(res.n_on_ball[s]) == int(out.sum()) and int(res.n_active[s]) == int((lam > 0.0).sum()) and res.residual[s] <= TOL


# ---------------------------------------------------------------- the three-encounter arc and the coupled scene against the restatement
# |device - restatement| measured on the first run on an MI355X (the tests print them), asserted at 3 x.  The two differ in their
# integrators (the device's discretiser and flight against the CPU oracle's) and in the arc itself (flown by the device here).
#   arc:     d0 history 3.09e-7 m, tca history 2.27e-11 s, terminal history 1.49e-13, final du / max |du| 2.93e-10
#   coupled: d0 history 3.47e-8 m
# (profiles/avoidance_refine.txt)
DEVICE_MEASURED = dict(arc_d0=3.09e-7, arc_tca=2.27e-11, arc_term=1.49e-13, arc_du=2.93e-10, coupled_d0=3.47e-8)


def allowed(key):
    m = DEVICE_MEASURED[key]
    assert m is not None, f"{key}: no measured figure recorded yet (see the printed differences)"
    return 3.0 * m


@functools.lru_cache(maxsize=None)
def arc_on_the_device(rounds):
    """three_encounters() with the arc as the device flies it (arc_on_device), the hold and u_max of the host loop -> result"""
    from mpconstellation_amd import avoidance_refine
    sc, pairs, rows, stage, cat = three_encounters()
    _, u_max = arc_loop(True, True, rounds)
    x = arc_on_device(sc["U"])
    M, T0, T1 = arc_grid()
    return avoidance_refine(pairs, TARGET, x[None], sc["U"][None], sc["units"][None], sc["span"][None], sc["consts"][None], M, T0, T1, rounds=rounds,
                            cat=cat[:3], u_max=u_max, hold_terminal=True, prop_max_step=AR.SCENE["prop_max_step"]), u_max


def test_three_encounter_arc_against_the_restatement():
    """histories and the final du against the restatement within 3 x the measured differences; the final shortfall and terminal
    deviation inside the host test's bounds; no node beyond u_max"""
    sc = three_encounters()[0]
    res, u_max = arc_on_the_device(ROUNDS)
    ref, _ = arc_loop(True, True)
    short, term = shortfall(res.d0_history), res.terminal_history[:, 0]
    diff = dict(arc_d0=np.abs(res.d0_history - ref["d0_history"]).max(), arc_tca=np.abs(res.tca_history - ref["tca_history"]).max(),
                arc_term=np.abs(res.terminal_history - ref["terminal_history"]).max(),
                arc_du=np.abs(res.du - ref["du"]).max() / np.abs(ref["du"]).max())
    print(f"status {res.status.tolist()}, rounds_done {res.rounds_done.tolist()}, iterations of the last solve {res.iters.tolist()}\nshortfall by pass {short}\n"
          f"terminal deviation by pass {term}\nd0 by pass\n{res.d0_history}\n|device - restatement|: {diff}")
    assert res.status.tolist() == [0] and res.rounds_done.tolist() == [ROUNDS]
    b = LOOP_BOUND[(True, True)]
    assert short[-1] <= b["shortfall"] and term[-1] <= b["terminal"]
    assert short[1] <= FLOWN_BOUND["shortfall"] and term[1] <= FLOWN_BOUND["terminal_hold"]
    ut = sc["U"] + res.du[0]
    assert (np.sqrt((ut * ut).sum(axis=0)) <= u_max[0] * (1.0 + 10.0 * TOL)).all() and res.n_on_ball[0] >= 1
    for k, d in diff.items():
        assert d <= allowed(k), (k, d)


def test_coupled_scene_on_the_device():
    """the host test's coupled scene: rounds = 0 leaves row 0 short by more than the uncoupled bound, rounds = 3 brings both rows
    within the refined loop's bound; the d0 history against the restatement"""
    from mpconstellation_amd import avoidance_refine
    pairs, mover, (Y, units, span, _), U, consts, (M, T0, T1) = coupled_scene()
    run = lambda rounds: avoidance_refine(pairs, TARGET, Y, U, units, span, consts, M, T0, T1, rounds=rounds, who=mover, hold_terminal=True,
                                          prop_max_step=AR.SCENE["prop_max_step"])
    r0, r3 = run(0), run(ROUNDS)
    ref = coupled_loop(ROUNDS)
    s0, s3 = np.maximum(TARGET - r0.d0_history[-1], 0.0) / TARGET, np.maximum(TARGET - r3.d0_history[-1], 0.0) / TARGET
    d = np.abs(r3.d0_history - ref["d0_history"]).max()
    print(f"rounds 0: flown {r0.d0_history[-1]}, shortfall {s0}; rounds 3: d0 by pass\n{r3.d0_history}\nshortfall {s3}; |device - restatement| d0 {d:.3e} m")
    assert r3.coupled.tolist() == [True, False] and r3.status.tolist() == [0, 0, 0] and r3.rounds_done.tolist() == [3, 3, -1]
    assert s0[0] > FLOWN_BOUND["shortfall"] and (s3 <= LOOP_BOUND[(True, True)]["shortfall"]).all()
    assert same_bits(r3.Y_flown[2], Y[2]) and not r3.du[2].any()
    assert d <= allowed("coupled_d0")


# ---------------------------------------------------------------- the bits
def refine_dev(sc, target, rounds, u_max, fill, optional):
    """mpcx_avoidance_refine_dev on the catalogue form with covariances and the hold, every device buffer a torch tensor: the workspace
    and every result pre-filled with `fill`; optional: ask for rows, tsens, rhs_rows, rhs_term -> dict of numpy arrays"""
    import torch
    from mpconstellation_amd import _ffi
    from mpconstellation_amd.constants import MU_EARTH
    from mpconstellation_amd.conjunction import DEFAULT_MAX_STEP
    lib, ctx = _ffi.load(), _ffi.context(0)
    Y, units, span, ns = sc["rows"]
    cY, cunits, cspan, cns, cP = sc["cat"]
    S, _, K = Y.shape
    n, D = len(sc["pairs"]), len(cY)
    g = grid_of(K)
    wsb = int(lib.mpcx_avoidance_refine_workspace_bytes(n, S, K, D, g["M"]))
    assert wsb > 0 and wsb % 8 == 0
    ws = filled(wsb // 8, fill)
    ins = [dev(sc["pairs"]), dev(np.zeros(n, dtype=np.int32)), None if ns is None else dev(ns), dev(Y), dev(sc["U"]), dev(units), dev(span), dev(sc["consts"]),
           dev(sc["P"]), dev(cns), dev(cY), dev(cunits), dev(cspan), dev(cP), dev(u_max)]
    shapes = dict(du=(S, 3, K), sat_out=(S, 8), row_out=(n, 5), rows=(n, 3, K), tsens=(S, 6, 3, K), Y_flown=(S, 7, K), pairs_flown=(n, 4),
                  d0=(rounds + 2, n), tca=(rounds + 2, n), term=(rounds + 2, S), rhs_rows=(n,), rhs_term=(S, 6))
    o = {k: filled(int(np.prod(sh)), fill).reshape(sh) for k, sh in shapes.items()}
    for k, m in (("status", S), ("row_status", n), ("rounds_done", S)):
        o[k] = torch.full((m,), -7, dtype=torch.int32, device=ws.device)
    opt = lambda k: _p(o[k] if optional else None)
    rc = lib.mpcx_avoidance_refine_dev(ctx, n, _p(ins[0]), _p(ins[1]), S, K, _p(ins[2]), _p(ins[3]), _p(ins[4]), _p(ins[5]), _p(ins[6]), _p(ins[7]), 0,
                                       DEFAULT_MAX_STEP, _p(ins[8]), D, cY.shape[2], _p(ins[9]), _p(ins[10]), _p(ins[11]), _p(ins[12]), _p(ins[13]),
                                       MU_EARTH, target, _p(ins[14]), 1, TOL, 50, g["M"], g["T0"], g["T1"], PROP_MAX_STEP, rounds, _p(o["du"]),
                                       _p(o["sat_out"]), _p(o["row_out"]), opt("rows"), opt("tsens"), _p(o["status"]), _p(o["row_status"]),
                                       _p(o["Y_flown"]), _p(o["pairs_flown"]), _p(o["d0"]), _p(o["tca"]), _p(o["term"]), _p(o["rounds_done"]),
                                       opt("rhs_rows"), opt("rhs_term"), _p(ws), _stream(torch))
    _ffi.check(rc, ctx, "avoidance_refine_dev")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def test_same_bits():
    """called twice; with and without the optional outputs; the _dev form in a workspace and result arrays full of NaN and of 1e300
    against the host form"""
    S, K, D = 3, 30, 3
    sc = scene(S, K, D, False)
    target = targets(K)[1]
    u_max = free_limits(sc, target, True, True, True, 0.9)
    a = refine(sc, target, 2, P=True, hold_terminal=True, u_max=u_max)
    assert (a.rounds_done == 2).any()
    b = refine(sc, target, 2, P=True, hold_terminal=True, u_max=u_max)
    assert bits(a) == bits(b) and same_bits(a.rows, b.rows) and same_bits(a.tsens, b.tsens) and same_bits(a.rhs_rows, b.rhs_rows) and same_bits(a.rhs_term, b.rhs_term)
    c = refine(sc, target, 2, P=True, hold_terminal=True, u_max=u_max, return_rows=False, return_terminal=False, return_rhs=False)
    assert c.rows is None and c.tsens is None and c.rhs_rows is None and bits(a) == bits(c)
    names = dict(du="du", sat_out="sat_out", row_out="row_out", status="status", row_status="row_status", Y_flown="Y_flown", pairs_flown="pairs_flown",
                 d0="d0_history", tca="tca_history", term="terminal_history", rounds_done="rounds_done")
    for fill, optional in (("nan-", True), ("big", False)):
        d = refine_dev(sc, target, 2, u_max, fill, optional)
        for k, attr in names.items():
            assert same_bits(d[k], getattr(a, attr)), (fill, k)
        if optional:
            for k in ("rows", "tsens", "rhs_rows", "rhs_term"):
                assert same_bits(d[k], getattr(a, k)), (fill, k)


def test_a_satellite_infeasible_at_pass_zero_stays_nan():
    """a thrust limit that forbids satellite s0's rows: INFEASIBLE at pass 0, NaN for good, it never flies and counts as not moving;
    its neighbours are refined with the bits they have when s0's rows are not in the list at all"""
    S, K, D = 3, 30, 3
    sc = scene(S, K, D, False)
    target = targets(K)[0]
    s0 = int(sc["pairs"][0, 0])
    others = sc["pairs"][:, 0] != s0
    assert others.any()
    u_max = np.full(S, np.inf); u_max[s0] = 1e-9
    res = refine(sc, target, 2, hold_terminal=True, u_max=u_max)
    alone = refine(dict(sc, pairs=sc["pairs"][others]), target, 2, hold_terminal=True, u_max=u_max)
    print(f"statuses {res.status.tolist()}, rounds_done {res.rounds_done.tolist()}; without satellite {s0}'s rows {alone.status.tolist()}, {alone.rounds_done.tolist()}")
    assert res.status[s0] == J.ST_INFEASIBLE and res.rounds_done[s0] == -1 and np.isnan(res.du[s0]).all() and np.isnan(res.sat_out[s0]).all()
    assert same_bits(res.Y_flown[s0], sc["rows"][0][s0]) and not res.terminal_history[:, s0].any()
    keep = np.arange(S) != s0
    assert (res.rounds_done[keep] == alone.rounds_done[keep]).all() and (res.rounds_done[keep] == 2).any()
    for name in ("du", "sat_out", "Y_flown"):
        assert same_bits(getattr(res, name)[keep], getattr(alone, name)[keep]), name
    assert same_bits(res.row_out[others], alone.row_out) and same_bits(res.d0_history[:, others], alone.d0_history)
    assert same_bits(res.pairs_flown[others], alone.pairs_flown) and same_bits(res.terminal_history[:, keep], alone.terminal_history[:, keep])


# ---------------------------------------------------------------- ConstellationMPC and the C ABI
def test_constellation_mpc_install_and_fly_plan():
    """ConstellationMPC.avoidance_refine(install=True) on arc_instance() returns what the by-hand call returns, bit for bit, holds
    Y_flown and U + du of the refined satellite as its plan, and fly_plan flies that table: the flown segment starts on it"""
    from mpconstellation_amd import conjunction as cj, propagate_batch, _ffi
    mpc, sc = arc_instance()
    K = AR.SCENE["K"]
    cat3 = three_encounters()[4][:3]
    U0 = mpc._plan[1].copy()
    w = mpc._screen_windows("plan", 4)[0]
    scr, res = mpc.avoidance_refine(20000.0, TARGET, rounds=2, catalogue=cat3, install=True, model="plan")
    from mpconstellation_amd.optimizer import DEFAULT_OPTIONS
    u_lim = np.asarray({**DEFAULT_OPTIONS, **mpc.OPTIONS(mpc.horizon), **mpc.options}["u_lim"], dtype=np.float64)
    u_max = np.ascontiguousarray(np.broadcast_to(u_lim[..., 1], (2,)))
    hand = cj.avoidance_refine(scr, TARGET, w["Y"], U0, w["units"], w["span"], mpc.consts, w["M"], w["T0"], w["T1"], rounds=2, ns=w["ns"], cat=cat3,
                               u_max=u_max)
    print(f"pairs {scr.pairs[:, :2].tolist()}, statuses {res.status.tolist()}, rounds_done {res.rounds_done.tolist()}, d0 by pass {res.d0_history.tolist()}")
    assert scr.pairs[:, :2].tolist() == [[1.0, 0.0], [1.0, 1.0], [1.0, 2.0]] and res.status.tolist() == [0, 0] and res.rounds_done.tolist() == [-1, 2]
    assert bits(res) == bits(hand)
    assert np.array_equal(mpc._plan[1][1], U0[1] + res.du[1]) and np.array_equal(mpc._plan[1][0], U0[0]) and same_bits(mpc._plan[0], res.Y_flown)
    with pytest.raises(ValueError, match="model"):
        mpc.avoidance_refine(20000.0, TARGET, catalogue=cat3, model="reference")
    y0 = mpc._y0()
    mpc.fly_plan(tf=1)
    seg = mpc._seg_y[-1]
    n_eval = seg.shape[2]
    y, st, _ = propagate_batch(y0, 1, mpc.consts, (_ffi.CTRL_SEQUENCE, mpc._plan[1], K, mpc.plan_tf / mpc.interval), n_eval, mpc.include_drag,
                               mpc.include_J2, 0.001, Kus=mpc.plan_K, atmosphere=mpc.atmosphere)
    assert (st == 0).all() and same_bits(seg, y) and same_bits(np.ascontiguousarray(seg[:, :, 0]), np.ascontiguousarray(y0))


def test_c_abi():
    """the three exports exist; the workspace is 0 bytes for n < 1 (and S < 1, K < 2, D < 0, M < 2); rounds = -1 is MPCX_E_BADARG with
    a message, and nothing is written"""
    from mpconstellation_amd import _ffi
    lib, ctx = _ffi.load(), _ffi.context(0)
    for name in ("mpcx_avoidance_refine", "mpcx_avoidance_refine_dev", "mpcx_avoidance_refine_workspace_bytes"):
        assert hasattr(lib, name)
    wb = lib.mpcx_avoidance_refine_workspace_bytes
    assert wb(0, 3, 30, 3, 117) == 0 and wb(2, 0, 30, 3, 117) == 0 and wb(2, 3, 1, 3, 117) == 0 and wb(2, 3, 30, -1, 117) == 0 and wb(2, 3, 30, 3, 1) == 0
    assert wb(2, 3, 30, 0, 117) > lib.mpcx_avoidance_joint_workspace_bytes(2, 3, 30) and wb(2, 3, 30, 3, 117) > wb(2, 3, 30, 0, 117)
    S, K, n = 1, 8, 1
    d, i = lambda *sh: np.full(sh, 7.0), lambda m: np.full(m, 7, dtype=np.int32)
    o = dict(du=d(S, 3, K), sat_out=d(S, 8), row_out=d(n, 5), st=i(S), rst=i(n), Yo=d(S, 7, K), po=d(n, 4), h0=d(1, n), h1=d(1, n), h2=d(1, S), rd=i(S))
    pairs, Y, U = np.array([[0.0, 0.0, 1.0, 0.5]]), np.ones((S, 7, K)), np.zeros((S, 3, K))
    units, span, consts = np.ones((S, 2)), np.array([[0.0, 1.0]]), np.ones((S, 8))
    rc = lib.mpcx_avoidance_refine(ctx, n, _ffi.dptr(pairs), None, S, K, None, _ffi.dptr(Y), _ffi.dptr(U), _ffi.dptr(units), _ffi.dptr(span), _ffi.dptr(consts),
                                   0, 1e-2, None, 0, 0, None, None, None, None, None, 3.986004418e14, 100.0, None, 1, TOL, 50, 9, 0.0, 1.0, 1e-3, -1,
                                   _ffi.dptr(o["du"]), _ffi.dptr(o["sat_out"]), _ffi.dptr(o["row_out"]), None, None, _ffi.iptr(o["st"]), _ffi.iptr(o["rst"]),
                                   _ffi.dptr(o["Yo"]), _ffi.dptr(o["po"]), _ffi.dptr(o["h0"]), _ffi.dptr(o["h1"]), _ffi.dptr(o["h2"]), _ffi.iptr(o["rd"]),
                                   None, None)
    assert rc == -2 and all((v == 7).all() for v in o.values())
    with pytest.raises(Exception, match="rounds"):
        _ffi.check(rc, ctx, "avoidance_refine")
