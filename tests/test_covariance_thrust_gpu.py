"""The covariance with thrust execution errors on the device (csrc/covariance_thrust.hip) against its numpy restatement
(covariance_thrust_reference.py) fed the device's own A, B_kn, B_kp, against conjunction.covariance and itself (same bits), its
failure handling, and end to end on the planted encounter of test_avoidance_gpu.py.

Tolerance of the comparison with the restatement: the entrywise product bound run along the chain with gamma = 32 eps
(covariance_thrust_reference.chain_error_bound: collision_reference.chain_error_bound extended by the cross-covariance and the two
input terms), computed from the test's own inputs.  Measured when this file was written: the device sits at 0.027 .. 0.036 of it (every
case prints its figure)."""
import numpy as np
import pytest

import avoidance_reference as AR
import collision_reference as C
import covariance_thrust_reference as T

pytestmark = pytest.mark.gpu

EXEC = np.array([1e-4, 0.02, 1e-4, 0.01745, 1e-3])


def thrust_case(S, K, ragged):
    """test_collision_gpu.chain_case (S circular LEO orbits over 2000 s at K nodes; ragged: counts between 2 and K, the first is 2) with
    a thrust table of 0.02 standard_normal, every second satellite's first node and every third one's last node exactly zero, one node
    of each longer row at half of u_off; execution rows that differ by satellite, mass variances and noise densities that are zero
    for some satellites"""
    from test_collision_gpu import chain_case
    Y, units, span, ns, consts = chain_case(S, K, ragged)
    rng = np.random.default_rng(7 * S + K)
    U = 0.02 * rng.standard_normal((S, 3, K))
    counts = np.full(S, K) if ns is None else ns
    for s in range(S):
        nn = int(counts[s])
        U[s, :, nn:] = 1e300
        if s % 2 == 0:
            U[s, :, 0] = 0.0
        if s % 3 == 0:
            U[s, :, nn - 1] = 0.0
        if nn > 4:
            U[s, :, nn // 2] = np.array([0.3, -0.4, 0.0]) * EXEC[4]
    ex = EXEC[None, :] * (1.0 + 0.25 * np.arange(S))[:, None]
    mv = np.where(np.arange(S) % 2 == 1, 1e-4, 0.0)
    q = np.where(np.arange(S) % 3 == 1, 1e-6, 0.0)
    return dict(Y=Y, units=units, span=span, ns=ns, consts=consts, U=U, ex=ex, mv=mv, q=q)


@pytest.mark.parametrize("S,K,ragged,drag,J2", [(1, 2, False, False, False), (3, 3, False, False, True), (5, 30, False, False, False),
                                               (5, 30, True, True, True)])
def test_chain_against_the_restatement(S, K, ragged, drag, J2):
    """|P - restated| <= E and |Pm - restated| <= Em entrywise; P symmetric to the bit; node 0 is P0 and m_var0; nodes past ns zero"""
    from mpconstellation_amd import covariance_thrust, _ffi
    from test_avoidance_gpu import device_stage
    c = thrust_case(S, K, ragged)
    flags = (_ffi.FLAG_DRAG if drag else 0) | (_ffi.FLAG_J2 if J2 else 0)
    A, Bn, Bp = device_stage(c["Y"], c["U"], c["units"], c["span"], c["consts"], c["ns"], flags)
    chain = (A, Bn, Bp, c["U"], c["units"], c["span"], C.P0_TEST, c["ex"])
    ref, refm, ref_status = T.covariance_thrust_chain(*chain, q=c["q"], m_var0=c["mv"], ns=c["ns"])
    E, Em = T.chain_error_bound(*chain, q=c["q"], m_var0=c["mv"], ns=c["ns"])
    P, Pm, status = covariance_thrust(c["Y"], c["units"], c["span"], c["consts"], C.P0_TEST, c["U"], c["ex"], mass_var0=c["mv"], ns=c["ns"], q=c["q"],
                                      include_drag=drag, include_J2=J2, return_status=True, return_mass=True)
    assert (status == 0).all() and (ref_status == 0).all()
    worst = max((np.abs(P - ref) / np.where(E > 0.0, E, 1.0)).max(), (np.abs(Pm - refm) / np.where(Em > 0.0, Em, 1.0)).max())
    print(f"S {S} K {K} ragged {ragged} drag {drag} J2 {J2}: worst |device - restated| / bound = {worst:.3f}")
    assert (np.abs(P - ref) <= E).all() and (np.abs(Pm - refm) <= Em).all()
    assert np.array_equal(P, np.transpose(P, (0, 1, 3, 2)))
    assert np.array_equal(P[:, 0], np.broadcast_to(C.P0_TEST, (S, 6, 6))) and np.array_equal(Pm[:, 0, 6], c["mv"]) and (Pm[:, 0, :6] == 0.0).all()
    assert (Pm[:, 1, 6] >= c["mv"] * (1.0 - 1e-9)).all() and (Pm[1:, 1, 6] > 0.0).all()      # the mass variance is carried, thrust errors add to it
    if c["ns"] is not None:
        for s in range(S):
            n = c["ns"][s]
            assert (P[s, n:] == 0.0).all() and (Pm[s, n:] == 0.0).all() and (P[s, n - 1] != 0.0).any()


def test_same_bits():
    """A mixed batch: the satellites whose execution row is zero and whose mass variance is 0 have conjunction.covariance's P, the
    others do not; a satellite alone and in the batch; devices=[0, 0]; with and without Pm; a second context; the _dev call over a
    workspace and results filled with garbage."""
    import torch
    from mpconstellation_amd import covariance, covariance_thrust, conjunction as cj, _ffi
    from dev_solve import dev, filled, same_bits, _p, _stream
    S, K = 5, 30
    c = thrust_case(S, K, True)
    zero = np.array([True, False, True, False, True])
    ex, mv = np.where(zero[:, None], 0.0, c["ex"]), np.where(zero, 0.0, 1e-4)
    fixed = dict(ns=c["ns"], q=c["q"], include_J2=True)
    plain, pst = covariance(c["Y"], c["units"], c["span"], c["consts"], C.P0_TEST, U=c["U"], return_status=True, **fixed)
    run = lambda **kw: covariance_thrust(c["Y"], c["units"], c["span"], c["consts"], C.P0_TEST, c["U"], ex, mass_var0=mv, return_status=True, **fixed, **kw)
    P, Pm, st = run(return_mass=True)
    assert (st == 0).all() and (pst == 0).all()
    for s in range(S):
        n = c["ns"][s]
        assert np.array_equal(P[s], plain[s]) == bool(zero[s]), s
        if zero[s]:
            assert (Pm[s] == 0.0).all()
        elif n > 2:
            assert (np.abs(P[s, n - 1] - plain[s, n - 1]) > 1e-9 * np.abs(plain[s, n - 1])).any()
    # a zero execution row for everybody, with the thrust table's garbage behind the counts: the whole batch is covariance's
    Pz = covariance_thrust(c["Y"], c["units"], c["span"], c["consts"], C.P0_TEST, c["U"], np.zeros(5), **fixed)
    assert np.array_equal(Pz, plain)
    drag = dict(ns=c["ns"], q=c["q"], include_drag=True, include_J2=True)      # (with drag the mass column of A is longer, the mass row still zero)
    assert np.array_equal(covariance_thrust(c["Y"], c["units"], c["span"], c["consts"], C.P0_TEST, c["U"], np.zeros(5), **drag),
                          covariance(c["Y"], c["units"], c["span"], c["consts"], C.P0_TEST, U=c["U"], **drag))
    # alone and in the batch
    for s in (1, 4):
        one = covariance_thrust(c["Y"][s:s + 1], c["units"][s:s + 1], c["span"][s:s + 1], c["consts"][s:s + 1], C.P0_TEST, c["U"][s:s + 1], ex[s:s + 1],
                                mass_var0=mv[s:s + 1], ns=c["ns"][s:s + 1], q=c["q"][s:s + 1], include_J2=True)
        assert same_bits(one[0], P[s])
    # two contexts of one device, without Pm, another context
    P2, Pm2, st2 = run(return_mass=True, devices=[0, 0])
    assert same_bits(P2, P) and same_bits(Pm2, Pm) and same_bits(st2, st)
    P3, st3 = run()
    assert same_bits(P3, P)
    out = dict(P=np.empty_like(P), Pm=np.empty_like(Pm), status=np.zeros(S, dtype=np.int32))
    cj._covariance_thrust_call(c["Y"], c["units"], c["span"], c["consts"], cj._check_p0(C.P0_TEST, S), c["U"], c["ns"], c["q"], _ffi.as_f64(ex), mv,
                               device=0, slot=1, out=out, flags=_ffi.FLAG_J2, max_step=cj.DEFAULT_MAX_STEP, atmosphere=None)
    assert same_bits(out["P"], P) and same_bits(out["Pm"], Pm)
    # the _dev call, every device buffer a torch tensor, workspace and results pre-filled
    lib, ctx = _ffi.load(), _ffi.context(0)
    wsb = int(lib.mpcx_covariance_thrust_workspace_bytes(S, K))
    assert wsb >= S * (K - 1) * _ffi.STAGE_DOUBLES * 8 and wsb % 8 == 0
    ins = [dev(a) for a in (c["ns"], c["Y"], c["U"], c["units"], c["span"], c["consts"], np.broadcast_to(C.P0_TEST, (S, 6, 6)), c["q"], ex, mv)]
    for fill in ("zero", "big", "nan+"):
        ws, dP, dPm = filled(wsb // 8, fill), filled(S * K * 36, fill), filled(S * K * 7, fill)
        dst = torch.full((S,), -7, dtype=torch.int32, device=ws.device)
        rc = lib.mpcx_covariance_thrust_batch_dev(ctx, S, K, _p(ins[0]), _p(ins[1]), _p(ins[2]), _p(ins[3]), _p(ins[4]), _p(ins[5]), _ffi.FLAG_J2,
                                                  cj.DEFAULT_MAX_STEP, _p(ins[6]), _p(ins[7]), _p(ins[8]), _p(ins[9]), _p(dP), _p(dPm), _p(dst), _p(ws),
                                                  _stream(torch))
        _ffi.check(rc, ctx, "mpcx_covariance_thrust_batch_dev")
        torch.cuda.synchronize()
        assert same_bits(dP.cpu().numpy().reshape(S, K, 6, 6), P) and same_bits(dPm.cpu().numpy().reshape(S, K, 7), Pm), fill
        assert dst.cpu().numpy().tolist() == [0] * S


def test_per_satellite_failures_leave_the_neighbours_alone():
    """every status in one call -- a count of 1 (BADK), a non-finite P0, a negative and a non-finite execution entry, a negative mass
    variance (NUMERIC) -- each NaN in P and Pm at all K nodes; the satellites between them bit for bit what they are in a batch of
    their own; the statuses are the restatement's"""
    from mpconstellation_amd import covariance_thrust
    S, K = 7, 8
    c = thrust_case(S, K, False)
    P0 = np.broadcast_to(C.P0_TEST, (S, 6, 6)).copy(); P0[2, 1, 4] = np.inf; P0[0, 5, 0] = np.nan      # (0: below the diagonal, never read)
    ex = c["ex"].copy(); ex[3, 1] = -0.1; ex[4, 4] = np.nan
    mv = c["mv"].copy(); mv[5] = -1e-6
    ns = np.array([8, 1, 8, 8, 8, 8, 5], dtype=np.int32)
    run = lambda at: covariance_thrust(c["Y"][at], c["units"][at], c["span"][at], c["consts"][at], P0[at], c["U"][at], ex[at], mass_var0=mv[at], ns=ns[at],
                                       q=c["q"][at], return_status=True, return_mass=True)
    P, Pm, st = run(np.arange(S))
    assert st.tolist() == [0, T.ST_BADK, T.ST_NUMERIC, T.ST_NUMERIC, T.ST_NUMERIC, T.ST_NUMERIC, 0]
    bad = st != 0
    assert np.isnan(P[bad]).all() and np.isnan(Pm[bad]).all() and np.isfinite(P[~bad]).all() and np.isfinite(Pm[~bad]).all()
    Pa, Pma, sta = run(np.array([0, 6]))
    assert (sta == 0).all() and np.array_equal(Pa, P[[0, 6]]) and np.array_equal(Pma, Pm[[0, 6]])
    z = np.zeros((S, K - 1, 7, 7)), np.zeros((S, K - 1, 7, 3)), np.zeros((S, K - 1, 7, 3))
    _, _, ref_status = T.covariance_thrust_chain(*z, c["U"], c["units"], c["span"], P0, ex, q=c["q"], m_var0=mv, ns=ns)
    assert np.array_equal(ref_status, st)
    # covariance's own failures come first: an empty span with a bad execution row is BADK
    sp = c["span"].copy(); sp[3] = (5.0, 5.0)
    _, st = covariance_thrust(c["Y"], c["units"], sp, c["consts"], C.P0_TEST, c["U"], ex, return_status=True)
    assert st.tolist() == [0, 0, 0, T.ST_BADK, T.ST_NUMERIC, 0, 0]


def test_c_abi_refusals():
    from mpconstellation_amd import _ffi
    lib, ctx = _ffi.load(), _ffi.context(0)
    S, K = 2, 5
    d, i = _ffi.dptr, _ffi.iptr
    arrays = dict(X=np.ones((S, 7, K)), U=np.zeros((S, 3, K)), units=np.ones((S, 2)), span=np.array([[0.0, 1.0]] * S), consts=np.ones((S, 8)),
                  P0=np.zeros((S, 6, 6)), exec=np.zeros((S, 5)), P=np.zeros((S, K, 6, 6)))
    st = np.zeros(S, dtype=np.int32)

    def call(S=S, K=K, flags=0, max_step=1e-2, null=None):
        p = {k: (None if k == null else d(v)) for k, v in arrays.items()}
        return lib.mpcx_covariance_thrust_batch(ctx, S, K, None, p["X"], p["U"], p["units"], p["span"], p["consts"], flags, max_step, p["P0"], None,
                                                p["exec"], None, p["P"], None, None if null == "status" else i(st))
    for bad in [dict(S=0), dict(K=1), dict(max_step=0.0), dict(max_step=-1.0), dict(flags=4), dict(flags=64), dict(flags=_ffi.FLAG_ATMO)] + [dict(null=k) for k in list(arrays) + ["status"]]:
        assert call(**bad) == -2, bad
        assert b"covariance_thrust" in lib.mpcx_last_error(ctx), (bad, lib.mpcx_last_error(ctx))
    w = lib.mpcx_covariance_thrust_workspace_bytes
    assert w(0, 5) == 0 and w(2, 1) == 0 and w(2, 5) >= 2 * 4 * _ffi.STAGE_DOUBLES * 8
    assert lib.mpcx_covariance_thrust_batch_dev(ctx, S, K, None, *[None] * 5, 0, 1e-2, *[None] * 9) == -2
    assert b"covariance_thrust" in lib.mpcx_last_error(ctx)


def test_end_to_end_a_four_sigma_burn_is_not_four_sigma_under_execution_errors():
    """The planted scene of test_avoidance_gpu.py's end-to-end test: screen_against -> covariance -> avoidance at 4 sigma -> apply, the
    changed plan flown, then collision_probability twice on the same screen: with covariance of the changed plan, and with
    covariance_thrust at 2 % magnitude and 0.01745 rad (1 degree) pointing error.  The frame is the same (miss and relative speed to
    the bit); the Mahalanobis distance with execution errors is strictly below the one without, and below 4; P_thrust - P_plain is
    positive semidefinite at every node to the rounding bound (the smallest eigenvalue against the Frobenius norms of the two chains'
    entrywise bounds).  Measured when this file was written (the test prints them): 3.999921 sigma without execution errors,
    1.973270 sigma with them; Pc 3.7e-7 and 6.8e-5."""
    from mpconstellation_amd import screen_against, covariance, covariance_thrust, collision_probability, avoidance
    from test_avoidance_gpu import arc_on_device, device_stage, scale_constants
    a = AR.arc_setup()
    K = AR.SCENE["K"]
    x = arc_on_device(a["U"])
    hn = (a["span"][1] - a["span"][0]) / (K - 1)
    cy, cu, cspan = AR.planted_object(dict(a, x=x), a["span"][0] + 20.37 * hn)
    units, span, consts = a["units"][None], a["span"][None], a["consts"][None]
    cY, cunits, cspans = cy[None], cu[None], cspan[None]
    P0 = np.diag([40.0 ** 2] * 3 + [0.02 ** 2] * 3)
    cP = covariance(cY, cunits, cspans, scale_constants(cunits[:, 0]), P0)
    grid = dict(M=4 * (K - 1) + 1, T0=float(span[0, 0]), T1=float(span[0, 1]), threshold=5000.0)
    screened = lambda x: screen_against(Y=x[None], units=units, span=span, cat_Y=cY, cat_units=cunits, cat_span=cspans, **grid)
    prob = lambda scr, x, P: collision_probability(scr, 5.0, x[None], units, span, P, cat=(cY, cunits, cspans, cP, 5.0))
    scr = screened(x)
    P = covariance(x[None], units, span, consts, P0, U=a["U"][None])
    av = avoidance(scr, 4.0, x[None], a["U"][None], units, span, consts, P=P, cat=(cY, cunits, cspans, cP))
    assert av.status.tolist() == [0] and abs(av.d1[0] - 4.0) <= 1e-9
    U2 = av.apply(a["U"][None], 0)[0]
    x2 = arc_on_device(U2)
    scr2 = screened(x2)
    ex = np.array([0.0, 0.02, 0.0, 0.01745, 0.0])
    P_plain = covariance(x2[None], units, span, consts, P0, U=U2[None])
    P_thrust, st = covariance_thrust(x2[None], units, span, consts, P0, U2[None], ex, return_status=True)
    col, col_t = prob(scr2, x2, P_plain), prob(scr2, x2, P_thrust)
    print(f"re-flown encounter: miss {col.miss[0]:.2f} m; without execution errors {col.mahalanobis[0]:.6f} sigma, Pc {col.pc[0]:.3e}; with 2 % and "
          f"1 degree {col_t.mahalanobis[0]:.6f} sigma, Pc {col_t.pc[0]:.3e}; sigma {col.sigma[0]} -> {col_t.sigma[0]} m")
    assert st.tolist() == [0] and col.status.tolist() == [0] and col_t.status.tolist() == [0]
    assert col.miss[0] == col_t.miss[0] and col.speed[0] == col_t.speed[0]
    assert col_t.mahalanobis[0] < col.mahalanobis[0] and col_t.mahalanobis[0] < 4.0
    assert col_t.pc[0] > col.pc[0]
    A, Bn, Bp = device_stage(x2[None], U2[None], units, span, consts)
    Et, _ = T.chain_error_bound(A, Bn, Bp, U2[None], units, span, P0, ex)
    Ep = C.chain_error_bound(A, units, span, P_plain)
    for k in range(K):
        w = np.linalg.eigvalsh(P_thrust[0, k] - P_plain[0, k])
        assert w.min() >= -(np.linalg.norm(Et[0, k]) + np.linalg.norm(Ep[0, k])), (k, w)
    assert np.array_equal(P_thrust[0, 0], P_plain[0, 0]) and np.linalg.eigvalsh(P_thrust[0, -1] - P_plain[0, -1]).max() > 0.0
