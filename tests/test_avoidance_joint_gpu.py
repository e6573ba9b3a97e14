"""The joint avoidance step on the device (csrc/avoidance_joint.hip): its rows and terminal sensitivities against mpcx_avoidance's own
bits and the numpy restatement (avoidance_joint_reference.py), the KKT conditions of every solved satellite checked on the host in
float64 from what the call returns, its du against the restatement's on the device's own rows, the special cases, the bits across
forms, and end to end: three planted encounters screened, opened to 4 sigma under a thrust limit with the terminal state held, flown
again and screened again.  Scenes, stage records and the arc come from test_avoidance_gpu.py and the host tests."""
import functools

import numpy as np
import pytest

import avoidance_joint_reference as J
import avoidance_reference as AR
import collision_reference as C
from test_avoidance_gpu import scene, union_of, device_stage, scale_constants, arc_on_device
from test_avoidance_joint_host import QP_BOUND, FLOWN_BOUND

pytestmark = pytest.mark.gpu

TOL = 1e-10
SCENES = [(5, 30, 9, False), (6, 70, 9, True), (4, 5, 6, False)]        # (S, K, D, ragged); K = 5: none of its encounters at the last node


def targets(K):
    # rows of 5 nodes over 3000 s interpolate a circle so badly that the planted pairs are up to 1e6 m apart (test_avoidance_gpu.py)
    return (1000.0, 6.0) if K >= 30 else (1.0e7, 1.0e5)


def run(sc, target, P=False, cat=True, pairs=None, **kw):
    from mpconstellation_amd import avoidance_joint
    Y, units, span, ns = sc["rows"]
    c = None
    if cat:
        cY, cunits, cspan, cns, cP = sc["cat"]
        c = (cY, cunits, cspan, cP, cns) if P else (cY, cunits, cspan, cns)
    kw.setdefault("return_rows", True); kw.setdefault("return_terminal", True)
    return avoidance_joint(sc["pairs"] if pairs is None else pairs, target, Y, sc["U"], units, span, sc["consts"], ns=ns, P=sc["P"] if P else None,
                           cat=c, **kw)


def restated(sc, stage, target, res, P=False, cat=True, pairs=None, own_rows=True, **kw):
    """the restatement on the same inputs; own_rows: fed the device's own rows and terminal sensitivities"""
    c = None
    if cat:
        cY, cunits, cspan, cns, cP = sc["cat"]
        c = (cY, cunits, cspan, cns, cP if P else None)
    extra = dict(a_rows=res.rows, T=res.tsens) if own_rows else {}
    return J.avoidance_joint(sc["pairs"] if pairs is None else pairs, res.mover, sc["rows"], sc["U"], stage, target, P=sc["P"] if P else None, cat=c,
                             **extra, **kw)


@functools.lru_cache(maxsize=None)
def solved(S, K, D, ragged, P, hold, ball):
    """one scene solved on the device (u_max: 0.9 x each satellite's largest |ubar + du| without a ball) -> (scene, stage, result, u_max)"""
    sc = scene(S, K, D, ragged)
    Y, units, span, ns = sc["rows"]
    stage = device_stage(Y, sc["U"], units, span, sc["consts"], ns)
    target = targets(K)[1 if P else 0]
    u_max = None
    if ball:
        free = run(sc, target, P=P, hold_terminal=hold, return_rows=False, return_terminal=False)
        u_max = np.where(free.status == 0, 0.9 * free.umax, np.inf)
        u_max[free.n_rows == 0] = np.inf
    return sc, stage, run(sc, target, P=P, hold_terminal=hold, u_max=u_max), u_max, target


def terminal_bound(A, nn, K, gamma=AR.GAMMA):
    """entrywise product bound along the terminal sweep, in the manner of avoidance_reference.sweep_error_bound (exact seeds)"""
    aA = np.abs(A)
    true = {nn - 1: np.hstack([np.eye(6), np.zeros((6, 1))])}
    E = {nn - 1: np.zeros((6, 7))}
    for m in range(nn - 2, -1, -1):
        true[m] = true[m + 1] @ A[m]
        E[m] = E[m + 1] @ aA[m] + gamma * (np.abs(true[m + 1]) @ aA[m])
    return true, E


@pytest.mark.parametrize("S,K,D,ragged", SCENES)
def test_rows_and_terminal_sensitivities(S, K, D, ragged):
    """rows without covariances = mpcx_avoidance's sens[:, slot, 0] bit for bit (catalogue form, and the all-pairs form with a mixed
    mover list against who='both'); with covariances within the entrywise bounds of the restatement; tsens within the product bound
    of the restatement fed the device's own A, B_kn, B_kp"""
    from mpconstellation_amd import avoidance
    sc = scene(S, K, D, ragged)
    Y, units, span, ns = sc["rows"]
    cY, cunits, cspan, cns, cP = sc["cat"]
    T_m, T_s = targets(K)
    res = run(sc, T_m, hold_terminal=True)
    av = avoidance(sc["pairs"], T_m, Y, sc["U"], units, span, sc["consts"], ns=ns, cat=(cY, cunits, cspan, cns), return_sensitivities=True)
    assert np.array_equal(res.row_status, av.status) and (res.row_status == 0).all()
    assert res.rows.tobytes() == np.ascontiguousarray(av.sens[:, 0, 0]).tobytes()
    assert np.array_equal(res.d0, av.d0)
    un = union_of(sc)
    uY, uunits, uspan, uns = un["rows"]
    mover = (np.arange(len(un["pairs"])) % 2).astype(np.int32)
    resu = run(un, T_m, cat=False, who=mover, hold_terminal=False)
    avu = avoidance(un["pairs"], T_m, uY, un["U"], uunits, uspan, un["consts"], ns=uns, who="both", return_sensitivities=True)
    assert (resu.row_status == 0).all()
    assert resu.rows.tobytes() == np.ascontiguousarray(avu.sens[np.arange(len(mover)), mover, 0]).tobytes()
    # with covariances: a = q_1 g[0] + q_2 g[1]; g within Es of the restatement; q from W = C_2^-1, C_2 good to 1e-10 relative
    # (test_collision_gpu.py) in a frame that two evaluations of the positions turn by 2 x POSITION_ALLOWANCE / |m|: 8 cond(W) times that
    stage = device_stage(Y, sc["U"], units, span, sc["consts"], ns)
    resP = run(sc, T_s, P=True, hold_terminal=True)
    enc = J.encounter_rows(sc["pairs"], None, sc["rows"], stage, T_s, P=sc["P"], cat=(cY, cunits, cspan, cns, cP))
    _, _, _, _, (_, _, Es) = AR.avoidance(sc["pairs"], sc["rows"], stage, T_s, "i", P=sc["P"], cat=(cY, cunits, cspan, cns, cP), with_bounds=True)
    q = np.abs(enc["q"])
    q_err = 8.0 * np.linalg.cond(enc["W"]) * (1e-10 + 2.0 * AR.POSITION_ALLOWANCE / enc["mn"] + 1e-12) * q.max(axis=1)
    Ea = q[:, 0, None, None] * Es[:, 0, 0] + q[:, 1, None, None] * Es[:, 0, 1] + q_err[:, None, None] * (np.abs(enc["g"][:, 0]) + np.abs(enc["g"][:, 1]))
    d = np.abs(resP.rows - enc["a"])
    print(f"S {S} K {K}: rows with covariances, worst |device - restated| / bound {np.max(d / np.where(Ea > 0, Ea, 1.0)):.3e}")
    assert (resP.row_status == 0).all() and (d <= Ea).all()
    assert np.allclose(resP.d0, enc["d0"], rtol=1e-8, atol=0.0)
    # terminal sensitivities of every satellite that has rows and whose problem was set up
    A, Bn, Bp = stage
    counts = np.full(S, K) if ns is None else ns
    worst = 0.0
    for s in np.flatnonzero(res.n_rows > 0):
        nn = int(counts[s])
        Tref = J.terminal_sens(A[s], Bn[s], Bp[s], nn, K)
        true, E = terminal_bound(A[s], nn, K)
        Eg = np.zeros((6, 3, K))
        for m in range(nn):
            if m <= nn - 2:
                Eg[:, :, m] += E[m + 1] @ np.abs(Bn[s][m]) + AR.GAMMA * (np.abs(true[m + 1]) @ np.abs(Bn[s][m]))
            if m >= 1:
                Eg[:, :, m] += E[m] @ np.abs(Bp[s][m - 1]) + AR.GAMMA * (np.abs(true[m]) @ np.abs(Bp[s][m - 1]))
        dT = np.abs(res.tsens[s] - Tref)
        worst = max(worst, float(np.max(dT / np.where(Eg > 0, Eg, 1.0))))
        assert (dT <= Eg).all() and not res.tsens[s][:, :, nn:].any() and res.tsens[s].any()
        assert res.tsens[s].tobytes() == resP.tsens[s].tobytes()
    print(f"S {S} K {K}: tsens, worst |device - restated| / bound {worst:.3e}")
    assert not res.tsens[res.n_rows == 0].any()


def kkt(sc, res, u_max, target, hold):
    """the KKT conditions of every satellite whose status is OK, in float64 from du, lambda, rows, tsens; returns how many were checked"""
    Y, units, span, ns = sc["rows"]
    S, _, K = Y.shape
    counts = np.full(S, K) if ns is None else ns
    checked = 0
    for s in np.flatnonzero((res.status == 0) & (res.n_rows > 0)):
        nn = int(counts[s])
        mine = np.flatnonzero(sc["pairs"][:, 0] == s)
        D, w, c = J.effort_weights(Y, units, span, ns, s)
        du, ub = res.du[s][:, :nn], sc["U"][s][:, :nn]
        a, lam = res.rows[mine][:, :, :nn], res.lam[mine]
        b = target - res.d0[mine]
        um = np.inf if u_max is None else u_max[s]
        slack = np.einsum("pcm,cm->p", a, du) - b
        assert (slack >= -10.0 * TOL * target).all(), (s, slack)
        assert (lam >= 0.0).all() and (slack[lam > 0.0] <= 10.0 * TOL * target).all(), (s, lam, slack)
        assert np.allclose(res.margin[mine], res.d0[mine] + slack + b, rtol=1e-12, atol=1e-9 * target)
        nrm = np.sqrt(((ub + du) ** 2).sum(axis=0))
        assert (nrm <= um * (1.0 + 10.0 * TOL)).all()
        v = np.einsum("p,pcm->cm", lam, a)
        y = np.zeros(6)
        if hold:
            T = res.tsens[s][:, :, :nn]
            assert np.abs(np.einsum("icm,cm->i", T, du)).max() <= 10.0 * TOL
            inside = nrm < um * (1.0 - 1e-9)
            Tm = T[:, :, inside].reshape(6, -1)
            y = np.linalg.lstsq(Tm.T, (D * du - v)[:, inside].ravel(), rcond=None)[0]
            v = v + np.einsum("i,icm->cm", y, T)
        pp, _, out = J.project(ub + v / D, um)
        err = np.abs(pp - ub - du).max()
        assert err <= 10.0 * TOL * np.abs(du).max(), (s, err, np.abs(du).max())
        assert int(res.n_on_ball[s]) == int(out.sum()) and int(res.n_active[s]) == int((lam > 0.0).sum()) and res.residual[s] <= TOL
        checked += 1
    return checked


@pytest.mark.parametrize("S,K,D,ragged", SCENES)
@pytest.mark.parametrize("P,hold,ball", [(True, True, True), (False, True, False), (False, False, True)])
def test_kkt_and_restatement(S, K, D, ragged, P, hold, ball):
    """every solved satellite meets the KKT conditions on the host; statuses and counts equal the restatement's on the device's own rows,
    du within the bound the host test measured between two independent solvers plus 10 tol"""
    sc, stage, res, u_max, target = solved(S, K, D, ragged, P, hold, ball)
    n_ok = kkt(sc, res, u_max, target, hold)
    ref = restated(sc, stage, target, res, P=P, u_max=u_max, hold_terminal=hold, tol=TOL)
    print(f"S {S} K {K} P {P} hold {hold} ball {ball}: statuses {res.status.tolist()}, rows {res.n_rows.tolist()}, active {res.n_active.tolist()}, on the ball "
          f"{res.n_on_ball.tolist()}, iterations {res.iters.tolist()} (restated {ref['sat_out'][:, J.AJ_ITERS].tolist()})")
    assert np.array_equal(res.status, ref["sat_status"]) and np.array_equal(res.row_status, ref["row_status"])
    if K == 5 and hold and ball:
        # 15 unknowns, 6 held terminal rows, 2 encounter rows: what is left cannot also take 10 % off the peak thrust.  The hold alone
        # and the ball alone are solved and checked at K = 5 by the other two parametrisations.
        assert n_ok == 0 and set(res.status[1:].tolist()) <= {J.ST_MAXITER, J.ST_INFEASIBLE}
    else:
        assert n_ok >= 1 and (not ball or (res.n_on_ball[res.status == 0] >= 1).any())
    ok = (res.status == 0) & (res.n_rows > 0)
    worst = 0.0
    for s in np.flatnonzero(ok):
        scale = np.abs(ref["du"][s]).max()
        err = np.abs(res.du[s] - ref["du"][s]).max()
        worst = max(worst, err / scale if scale > 0 else err)
        assert err <= (QP_BOUND + 10.0 * TOL) * scale
    print(f"    worst |du - restated du| / max |du| {worst:.3e}")
    bad = res.status != 0
    assert np.isnan(res.du[bad]).all() and np.isnan(res.sat_out[bad]).all() and not res.du[res.n_rows == 0].any()
    assert np.array_equal(res.n_rows[~bad], ref["sat_out"][~bad, J.AJ_ROWS]) and np.array_equal(res.n_active[~bad], ref["sat_out"][~bad, J.AJ_ACTIVE])
    rows_ok = ok[sc["pairs"][:, 0].astype(int)]
    assert np.isnan(res.row_out[~rows_ok, 1:]).all() and np.isfinite(res.row_out[rows_ok]).all()
    assert np.allclose(res.row_out[rows_ok], ref["row_out"][rows_ok], rtol=1e-6, atol=1e-6 * target)


def one_satellite(n_rows, K=30):
    """satellite 0 of a scene with n_rows catalogue objects planted on it, beside a second satellite with one: a scene dict"""
    sc = scene(2, K, n_rows + 1, False)
    pairs = sc["pairs"].copy()
    pairs[:, 0] = 0.0
    pairs[-1, 0] = 1.0
    return dict(sc, pairs=pairs)


def test_special_cases():
    """no rows; 8 rows OK and 9 rows BADK with the neighbour untouched; one row alone in closed form; a row the ball forbids; two
    identical rows (SINGULAR, as the header states); a failing pair makes its satellite NaN and no other"""
    sc9, sc8 = one_satellite(9), one_satellite(8)
    # the planted objects were made for other satellites: far away.  A target beyond them all makes every row active.
    r8 = run(sc8, 2.0e7, hold_terminal=False)
    r9 = run(sc9, 2.0e7, hold_terminal=False)
    print("8 rows:", r8.status.tolist(), r8.n_rows.tolist(), "9 rows:", r9.status.tolist())
    assert r8.status.tolist() == [0, 0] and r8.n_rows.tolist() == [8.0, 1.0] and (r8.margin >= 2.0e7 * (1.0 - 10 * TOL)).all()
    assert r9.status.tolist() == [J.ST_BADK, 0] and np.isnan(r9.du[0]).all() and np.isnan(r9.sat_out[0]).all() and (r9.row_status == 0).all()
    assert np.isnan(r9.row_out[:9, 1:]).all() and np.isfinite(r9.row_out[9]).all() and np.isfinite(r9.d0).all()
    alone = run(sc9, 2.0e7, pairs=sc9["pairs"][9:], hold_terminal=False)
    assert alone.du[1].tobytes() == r9.du[1].tobytes() and alone.row_out.tobytes() == r9.row_out[9:].tobytes() and not alone.du[0].any()
    assert alone.status.tolist() == [0, 0] and not alone.sat_out[0].any() and not alone.tsens.any()
    # a single row, no ball, no hold: du = D^-1 a^T b / (a D^-1 a^T)
    Y, units, span, ns = sc9["rows"]
    D, _, _ = J.effort_weights(Y, units, span, ns, 1)
    a, b = alone.rows[0], 2.0e7 - alone.d0[0]
    closed = (a / D) * (b / ((a * a) / D).sum())
    assert b > 0 and np.abs(alone.du[1] - closed).max() <= 10.0 * TOL * np.abs(closed).max()
    assert abs(alone.lam[0] - b / ((a * a) / D).sum()) <= 1e-9 * alone.lam[0] and alone.iters[1] == 1 and alone.n_active[1] == 1
    # a row the ball alone forbids
    reach = (0.5 * np.sqrt((a * a).sum(axis=0)) - (a * sc9["U"][1]).sum(axis=0)).sum()
    far = run(sc9, alone.d0[0] + 1.5 * reach, pairs=sc9["pairs"][9:], hold_terminal=False, u_max=0.5)
    near = run(sc9, alone.d0[0] + 0.5 * reach, pairs=sc9["pairs"][9:], hold_terminal=False, u_max=0.5)
    assert far.status.tolist() == [0, J.ST_INFEASIBLE] and np.isnan(far.du[1]).all() and near.status.tolist() == [0, 0] and near.umax[1] <= 0.5 * (1 + 10 * TOL)
    # two identical rows: SINGULAR (include/mpcx.h); the same row once is fine, and an identical row that is NOT active does no harm
    twin = sc9["pairs"][[9, 9]]
    rt = run(sc9, 2.0e7, pairs=twin, hold_terminal=False)
    assert rt.status.tolist() == [0, J.ST_SINGULAR] and np.isnan(rt.du[1]).all() and (rt.row_status == 0).all()
    slack_twin = run(sc9, 0.5 * alone.d0[0], pairs=twin, hold_terminal=False)
    assert slack_twin.status.tolist() == [0, 0] and not slack_twin.du.any() and not slack_twin.lam.any() and slack_twin.iters[1] == 0
    # a failing pair (time outside the span) makes its satellite NaN and no other
    bad = sc8["pairs"].copy(); bad[2, 3] = 1.0e6
    rb = run(sc8, 2.0e7, pairs=bad, hold_terminal=False)
    assert rb.row_status.tolist() == [0, 0, J.ST_BADK] + [0] * 6 and rb.status.tolist() == [J.ST_BADK, 0]
    assert np.isnan(rb.du[0]).all() and np.isnan(rb.row_out[2]).all() and np.isnan(rb.rows[2]).all() and rb.du[1].tobytes() == r8.du[1].tobytes()
    # a mover that is no satellite belongs to nobody
    lost = sc8["pairs"].copy(); lost[0, 0] = 7.0
    rl = run(sc8, 2.0e7, pairs=lost, hold_terminal=False)
    assert rl.row_status[0] == J.ST_BADK and rl.status.tolist() == [0, 0] and rl.n_rows.tolist() == [7.0, 1.0]


def bits(r):
    return (r.du.tobytes(), r.sat_out.tobytes(), r.row_out.tobytes(), r.status.tobytes(), r.row_status.tobytes())


def test_same_bits():
    """two contexts against one; with and without rows / tsens; unrelated pairs added to the list; the catalogue form against the
    all-pairs form of the union"""
    sc, stage, a, u_max, target = solved(5, 30, 9, False, True, True, True)
    assert (a.status == 0).any()
    b = run(sc, target, P=True, hold_terminal=True, u_max=u_max, devices=[0, 0])
    assert bits(a) == bits(b) and a.rows.tobytes() == b.rows.tobytes() and a.tsens.tobytes() == b.tsens.tobytes()
    c = run(sc, target, P=True, hold_terminal=True, u_max=u_max, return_rows=False, return_terminal=False, devices=[0, 0])
    assert c.rows is None and c.tsens is None and bits(a) == bits(c)
    # pairs of other satellites in front of, between and behind the rows of satellite s0 do not change s0's results
    s0 = int(sc["pairs"][0, 0])
    mine = sc["pairs"][:, 0] == s0
    d = run(sc, target, P=True, hold_terminal=True, u_max=u_max, pairs=sc["pairs"][mine])
    assert d.du[s0].tobytes() == a.du[s0].tobytes() and d.sat_out[s0].tobytes() == a.sat_out[s0].tobytes() and d.row_out.tobytes() == a.row_out[mine].tobytes()
    assert d.n_rows.sum() == mine.sum()
    # the union: satellites and objects as ONE constellation, j moved behind the satellites, nobody but the satellites moves
    un = union_of(sc)
    S = len(sc["rows"][0])
    um = np.concatenate([u_max, np.full(len(un["U"]) - S, np.inf)])
    e = run(un, target, P=True, cat=False, hold_terminal=True, u_max=um)
    assert e.du[:S].tobytes() == a.du.tobytes() and e.sat_out[:S].tobytes() == a.sat_out.tobytes() and e.row_out.tobytes() == a.row_out.tobytes()
    assert e.rows.tobytes() == a.rows.tobytes() and e.tsens[:S].tobytes() == a.tsens.tobytes() and not e.du[S:].any() and not e.coupled.any()


def arc_instance():
    """A ConstellationMPC of two satellites whose plan is installed by hand (update() would plan something else): satellite 1 is the
    host tests' thrusting arc as propagate_batch flies it, satellite 0 the same normalised plan in the units of an orbit 1400 km higher
    (every satellite sees MU = 4 pi^2 in its own units, so the plan is consistent there too) -- far from every planted object, so it
    has no rows; it is there so that a thrust limit taken from the wrong satellite shows.  -> (mpc, arc scene dict with x)"""
    from mpconstellation_amd import Satellite, ConstellationMPC
    a = AR.arc_setup()
    K, R0 = AR.SCENE["K"], AR.SCENE["radius"]
    x = arc_on_device(a["U"])
    sats = []
    for R in (R0 + 1.4e6, R0):
        v0 = np.sqrt(C.MU_EARTH / R)
        sats.append(Satellite(np.array([R, 0.0, 0.0]), np.array([0.0, v0 * np.cos(0.9), v0 * np.sin(0.9)]), 100.0))
    mpc = ConstellationMPC(sats, base_res=K, tf_horizon=1, tf_interval=1)
    assert np.array_equal(mpc.consts[1], a["consts"]) and mpc.scales[1].units["length"] == a["units"][0] and mpc.scales[1].units["time"] == a["units"][1]
    mpc._plan = (np.stack([x, x]), np.stack([a["U"], a["U"]]), None)
    mpc.plan_K, mpc.plan_tf = np.array([K, K], dtype=np.int32), np.array([AR.SCENE["tf"]] * 2)
    return mpc, dict(a, x=x)


def test_end_to_end_through_constellation_mpc():
    """The host tests' arc against three planted objects (first interval, mid-plan, last interval), end to end through a
    ConstellationMPC instance: ConstellationMPC.avoidance_joint screens the plan against the catalogue, propagates the covariance and
    solves with u_max from the instance's own per-satellite u_lim table (satellite 1: 0.8 of its free solution's peak, so the ball is
    active; satellite 0: a limit no manoeuvre of satellite 1 would fit in) and the terminal hold; then apply -> propagate again ->
    screen_against -> collision_probability.  Every pair reaches 4 sigma within the host test's shortfall bound, no node exceeds
    u_max, the terminal state stays within the host test's bound; and the method returns what the by-hand call with that table's
    upper column returns."""
    from mpconstellation_amd import screen_against, covariance, collision_probability, conjunction as cj
    mpc, sc = arc_instance()
    a, x = sc, sc["x"]
    K = AR.SCENE["K"]
    hn = (a["span"][1] - a["span"][0]) / (K - 1)
    times = [a["span"][0] + 0.6 * hn, a["span"][0] + 14.37 * hn, a["span"][0] + 28.45 * hn]
    units, span, consts = a["units"][None], a["span"][None], a["consts"][None]
    P0 = np.diag([40.0 ** 2] * 3 + [0.02 ** 2] * 3)
    grid = dict(M=4 * (K - 1) + 1, T0=float(span[0, 0]), T1=float(span[0, 1]), threshold=20000.0)

    def planted(misses):
        objs = [AR.planted_object(sc, t, miss=m, angle=ang) for t, m, ang in zip(times, misses, (1.1, 0.7, 2.0))]
        cY, cunits, cspans = np.stack([o[0] for o in objs]), np.stack([o[1] for o in objs]), np.stack([o[2] for o in objs])
        return cY, cunits, cspans, covariance(cY, cunits, cspans, scale_constants(cunits[:, 0]), P0)

    def assess(x, U, cat):
        """satellite 1 alone, by hand: the screen's list, the covariance and the collision probabilities"""
        cY, cunits, cspans, cP = cat
        scr = screen_against(Y=x[None], units=units, span=span, cat_Y=cY, cat_units=cunits, cat_span=cspans, **grid)
        P = covariance(x[None], units, span, consts, P0, U=U[None])
        col = collision_probability(scr, 5.0, x[None], units, span, P, cat=(cY, cunits, cspans, cP, 5.0))
        return scr, P, col
    # the objects 200 m away tell how many metres a sigma is at each encounter; then 0.97, 0.2 and 0.99 of 4 sigma away (the host test's scene in sigmas)
    _, _, col0 = assess(x, a["U"], planted((200.0, 200.0, 200.0)))
    assert col0.status.tolist() == [0, 0, 0]
    cat = planted(tuple(f * 4.0 * 200.0 / m for f, m in zip((0.97, 0.2, 0.99), col0.mahalanobis)))
    _, _, col = assess(x, a["U"], cat)
    assert (col.mahalanobis < 4.0).all()
    # through the instance: first with its default limit (no node on the ball), then with the per-satellite table
    scr, free = mpc.avoidance_joint(20000.0, 4.0, P0=P0, catalogue=cat)
    assert scr.pairs[:, :2].tolist() == [[1.0, 0.0], [1.0, 1.0], [1.0, 2.0]] and free.status.tolist() == [0, 0]
    assert free.n_rows.tolist() == [0.0, 3.0] and free.n_on_ball[1] == 0
    u_lim = np.array([[0.0, 1e-3 * free.umax[1]], [0.0, 0.8 * free.umax[1]]])
    mpc.options["u_lim"] = u_lim
    scr, res = mpc.avoidance_joint(20000.0, 4.0, P0=P0, catalogue=cat, return_rows=True)
    u_max = u_lim[1, 1]
    assert res.status.tolist() == [0, 0] and res.n_rows.tolist() == [0.0, 3.0] and res.n_on_ball[1] >= 1 and res.umax[1] <= u_max * (1.0 + 10.0 * TOL)
    assert np.allclose(res.d0, col.mahalanobis, rtol=1e-9) and (res.margin >= 4.0 * (1.0 - 10.0 * TOL)).all() and (res.d1 >= 4.0 * (1.0 - 1e-9)).all()
    w = mpc._screen_windows("plan", 4)[0]
    P = cj.covariance(w["Y"], w["units"], w["span"], mpc.consts, P0, U=mpc._plan[1], ns=w["ns"])
    hand = cj.avoidance_joint(scr, 4.0, w["Y"], mpc._plan[1], w["units"], w["span"], mpc.consts, ns=w["ns"], P=P, cat=cat, u_max=u_lim[:, 1],
                              return_rows=True)
    assert bits(res) == bits(hand) and res.rows.tobytes() == hand.rows.tobytes()
    swapped = cj.avoidance_joint(scr, 4.0, w["Y"], mpc._plan[1], w["units"], w["span"], mpc.consts, ns=w["ns"], P=P, cat=cat, u_max=u_lim[::-1, 1])
    assert swapped.status[1] != 0 or swapped.umax[1] <= u_lim[0, 1] * (1.0 + 10.0 * TOL)     # (the other satellite's limit is another problem)
    assert swapped.du.tobytes() != res.du.tobytes()
    U2 = res.apply(mpc._plan[1])
    assert np.array_equal(U2[0], a["U"]) and (np.sqrt((U2[1] * U2[1]).sum(axis=0)) <= u_max * (1.0 + 10.0 * TOL)).all()
    x2 = arc_on_device(U2[1])
    scr2, _, col2 = assess(x2, U2[1], cat)
    short = np.maximum(4.0 - col2.mahalanobis, 0.0) / 4.0
    dev = np.abs(x2[:6, -1] - x[:6, -1]).max()
    print(f"before: {col.mahalanobis} sigma, Pc {col.pc}; u_lim of the instance {u_lim[:, 1]} ({int(res.n_on_ball[1])} nodes on the ball, {int(res.n_active[1])} active rows, "
          f"{int(res.iters[1])} iterations, dv {res.dv[1]:.4f} m/s); predicted {res.d1} sigma, flown {col2.mahalanobis} sigma: worst shortfall {short.max():.3e} "
          f"(bound {FLOWN_BOUND['shortfall']:.3e}); terminal deviation {dev:.3e} (bound {FLOWN_BOUND['terminal_hold']:.3e}); Pc {col2.pc}")
    assert col2.status.tolist() == [0, 0, 0] and scr2.pairs[:, 1].tolist() == [0.0, 1.0, 2.0]
    assert short.max() <= FLOWN_BOUND["shortfall"] and dev <= FLOWN_BOUND["terminal_hold"]
    assert (col2.pc <= col.pc).all()
