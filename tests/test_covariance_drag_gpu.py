"""The covariance with an uncertain drag on the device: the drag column of the stage records (MPCX_FLAG_DRAG_COLUMN, csrc/discretize.hip)
against covariance_drag_reference.drag_column and against the records without the bit; the chain (csrc/covariance_drag.hip) against its
numpy restatement fed the device's own records, against conjunction.covariance_thrust / covariance and itself (same bits), its failure
handling and refusals; the sensitivity it propagates against flights with a scaled drag; and end to end on a planted encounter.

Tolerances.  The column: RTOL = 1e-10 under relerr, what tests/test_drag_model_gpu.py holds every column of these records to.  The
chain: the entrywise product bound run along the chain with gamma = 32 eps (covariance_drag_reference.chain_error_bound).  The flown
check: four times the flights' own disagreement between two difference quotients plus test_covariance_drag_host.py's quadrature figure.
Every case prints what it measured; the figures measured when this file was written are in the docstrings of the tests."""
import os

import numpy as np
import pytest

import avoidance_reference as AR
import collision_reference as C
import covariance_drag_reference as R
import covariance_thrust_reference as T

pytestmark = pytest.mark.gpu

RTOL = 1e-10                     # tests/test_drag_model_gpu.py
ARC_S_SCALE = 1e2                # the 100 kg arc of avoidance_reference.py at S x 1e2: the drag share (2e-4 of A) of the fixture's Hubble at S x 1e4
C_S = 5
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "drag_discretize.npz"))
K30 = ("tan_K30_tf1", "tan_K30_tf1_J2", "tan_K30_tf1_bigS", "tan_K30_tf1_bigS_J2")
EXEC = np.array([1e-4, 0.02, 1e-4, 0.01745, 1e-3])


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


# ---------------------------------------------------------------- the column
def gold(name):
    g = lambda k: GOLD[f"{k}_{name}"]
    return g("x"), g("u"), float(g("tf")), g("const")[None] if g("const").ndim == 1 else g("const"), bool(g("j2"))


def sliced(S, K, counts=None):
    """S satellites of K nodes cut out of the K = 30 golden trajectories: satellite s takes the columns 3 s .. 3 s + n - 1 of the
    plain (even s) or the drag-scaled (odd s) case with tf = (n - 1) / 29, so its intervals are the fixture's own; ragged: n = counts[s],
    NaN behind them (never read)"""
    x, u, tf, cst = np.full((S, 7, K), np.nan), np.full((S, 3, K), np.nan), np.zeros(S), np.zeros((S, 8))
    for s in range(S):
        gx, gu, _, gc, _ = gold("tan_K30_tf1_bigS" if s % 2 else "tan_K30_tf1")
        n = K if counts is None else int(counts[s])
        x[s, :, :n], u[s, :, :n], tf[s], cst[s] = gx[:, 3 * s:3 * s + n], gu[:, 3 * s:3 * s + n], (n - 1) / 29.0, gc[0]
    return x, u, tf, cst


def atmosphere(model):
    import drag_cases as D
    return D.models()["general"] if model == "general_J2" else None


def records(x, u, tf, cst, Ks, flags, column, atm=None):
    """the device's stage records [S][K-1][105] and status under flags (| MPCX_FLAG_DRAG_COLUMN), as enc_linearise asks for them"""
    from mpconstellation_amd import _ffi
    from dev_solve import discretize_stages
    if atm is not None:
        _ffi.atmosphere_context(0, 0, atm)
        flags |= _ffi.FLAG_ATMO
    stage, st = discretize_stages(x, u, tf, cst, Ks=Ks, Kus=Ks, flags=flags | (_ffi.FLAG_DRAG_COLUMN if column else 0))
    return stage.cpu().numpy(), st


def check_column(x, u, tf, cst, Ks, j2, atm, tag):
    """with and without the bit: A, B_kn, B_kp, xi to the bit, the Sigma slot differs and is drag_column's to RTOL"""
    import oracle_lib as O
    from mpconstellation_amd import _ffi
    flags = _ffi.FLAG_DRAG | (_ffi.FLAG_J2 if j2 else 0)
    plain, st0 = records(x, u, tf, cst, Ks, flags, False, atm)
    col, st1 = records(x, u, tf, cst, Ks, flags, True, atm)
    assert (st0 == 0).all() and (st1 == 0).all()
    worst = 0.0
    for s in range(x.shape[0]):
        n = x.shape[2] if Ks is None else int(Ks[s])
        a, b = plain[s, :n - 1], col[s, :n - 1]
        assert a[:, :91].tobytes() == b[:, :91].tobytes() and a[:, 98:].tobytes() == b[:, 98:].tobytes(), (tag, s)
        assert (a[:, 91:97] != b[:, 91:97]).all() and (b[:, 97] == 0.0).all(), (tag, s)
        G, _ = R.drag_column(x[s, :, :n], u[s, :, :n], float(tf[s]), cst[s], O.FLAG_DRAG | (O.FLAG_J2 if j2 else 0), atm)
        worst = max(worst, relerr(b[:, 91:98], G))
    print(f"{tag}: worst relerr of the drag column against the oracle's nodes {worst:.3e} (allowed {RTOL:.0e})")
    assert worst <= RTOL
    return col


@pytest.mark.parametrize("model", ["fixed", "fixed_J2", "general_J2"])
@pytest.mark.parametrize("shape", ["S1_K2", "S9_K2", "S3_K7_ragged"])
def test_drag_column_small_shapes(shape, model):
    """S = 1, K = 2; S = 9, K = 2 (more items than the 8 groups of a wave: the tail groups shadow); S = 3, K = 7 ragged with a count of 2.
    In the S = 9 batch a satellite alone gives the bits it has in the batch.  Measured: 9e-17 .. 7e-15."""
    S, K, counts = {"S1_K2": (1, 2, None), "S9_K2": (9, 2, None), "S3_K7_ragged": (3, 7, np.array([7, 2, 5], dtype=np.int32))}[shape]
    x, u, tf, cst = sliced(S, K, counts)
    atm, j2 = atmosphere(model), model != "fixed"
    col = check_column(x, u, tf, cst, counts, j2, atm, f"{shape} {model}")
    if S == 9:
        from mpconstellation_amd import _ffi
        one, st = records(x[4:5], u[4:5], tf[4:5], cst[4:5], None, _ffi.FLAG_DRAG | (_ffi.FLAG_J2 if j2 else 0), True, atm)
        assert st.tolist() == [0] and one[0].tobytes() == col[4].tobytes()


@pytest.mark.parametrize("name", K30 + ("tan_K30_tf1_bigS_J2+general",))
def test_drag_column_golden_cases(name):
    """the K = 30 golden cases under the fixed density, and the drag-scaled one under an Atmosphere.  Measured: 4e-16 .. 6e-15."""
    x, u, tf, cst, j2 = gold(name.split("+")[0])
    check_column(x[None], u[None], np.array([tf]), cst, None, j2, atmosphere("general_J2") if "+" in name else None, name)


def test_drag_column_refusals():
    """the bit without MPCX_FLAG_DRAG, with MPCX_FLAG_UNIFORM_STEPS, with MPCX_FLAG_RK23: MPCX_E_BADARG and "discretize" in the
    message, the status array untouched (nothing enqueued); the reference-layout call ignores the bit"""
    import torch
    from mpconstellation_amd import _ffi
    from dev_solve import dev, _p, _stream
    lib, ctx = _ffi.load(), _ffi.context(0)
    x, u, tf, cst = sliced(2, 3)
    d = [dev(a) for a in (x, u, tf, cst)]
    stage = torch.zeros((2, 2, _ffi.STAGE_DOUBLES), dtype=torch.float64, device=d[0].device)
    st = torch.full((2,), -7, dtype=torch.int32, device=d[0].device)
    for flags in (64, 64 | _ffi.FLAG_J2, 64 | _ffi.FLAG_DRAG | _ffi.FLAG_UNIFORM_STEPS | (5 << 8), 64 | _ffi.FLAG_DRAG | _ffi.FLAG_RK23):
        for ragged in (False, True):
            if ragged:
                rc = lib.mpcx_discretize_stages_ragged_dev(ctx, 2, 3, None, 3, None, _p(d[0]), _p(d[1]), _p(d[2]), _p(d[3]), flags, 1e-2, _p(stage), _p(st), _stream(torch))
            else:
                rc = lib.mpcx_discretize_stages_dev(ctx, 2, 3, 3, _p(d[0]), _p(d[1]), _p(d[2]), _p(d[3]), flags, 1e-2, _p(stage), _p(st), _stream(torch))
            assert rc == -2 and b"discretize" in lib.mpcx_last_error(ctx), (flags, ragged)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [-7, -7] and not stage.any()
    from test_avoidance_gpu import device_stage
    units, span = np.ones((2, 2)), np.stack([np.zeros(2), tf], axis=1)
    a = device_stage(x, u, units, span, cst, flags=_ffi.FLAG_DRAG)
    b = device_stage(x, u, units, span, cst, flags=_ffi.FLAG_DRAG | 64)
    assert all(p.tobytes() == q.tobytes() for p, q in zip(a, b))


# ---------------------------------------------------------------- the chain
def drag_case(S, K, ragged):
    """test_covariance_thrust_gpu.thrust_case -- its satellites have a mass of 1 kg, so under the fixed density their drag is 2e-4 of A
    as it stands, the share of the fixture's drag-scaled Hubble --, every fourth satellite's execution row zero, and density rows that
    differ by satellite: sigma 0.2, 0, 0.1, 0.3, 0.05, ... and tau inf, 600 s, a third of the node spacing, inf, ..."""
    from test_covariance_thrust_gpu import thrust_case
    c = thrust_case(S, K, ragged)
    c["ex"] = np.where((np.arange(S) % 4 == 2)[:, None], 0.0, c["ex"])
    counts = np.full(S, K) if c["ns"] is None else c["ns"]
    h = (c["span"][:, 1] - c["span"][:, 0]) / (counts - 1)
    sig = np.array([0.2, 0.0, 0.1, 0.3, 0.05])[np.arange(S) % 5]
    tau = np.where(np.arange(S) % 3 == 0, np.inf, np.where(np.arange(S) % 3 == 1, 600.0, h / 3.0))
    c["dens"] = np.stack([sig, tau], axis=1)
    return c


def device_blocks(c, flags, atm=None):
    """A, B_kn, B_kp, G of the device's own records with the drag column, for the restatement"""
    S, _, K = c["Y"].shape
    tf = (c["span"][:, 1] - c["span"][:, 0]) / c["units"][:, 1]
    rec, st = records(c["Y"], c["U"], tf, c["consts"], c["ns"], flags, True, atm)
    assert (st == 0).all()
    return (rec[:, :, :49].reshape(S, K - 1, 7, 7), rec[:, :, 49:70].reshape(S, K - 1, 7, 3), rec[:, :, 70:91].reshape(S, K - 1, 7, 3),
            np.ascontiguousarray(rec[:, :, 91:98]))


@pytest.mark.parametrize("S,K,ragged,J2", [(1, 2, False, False), (3, 3, False, True), (5, 30, True, True)])
def test_chain_against_the_restatement(S, K, ragged, J2):
    """|P - restated| <= E, |Pm - restated| <= Em, |Pb - restated| <= Eb entrywise; P symmetric to the bit; node 0 is (P0, m_var0,
    sigma^2); nodes past ns zero.  Measured: the device sits at 0.025 .. 0.030 of the bound."""
    from mpconstellation_amd import covariance_drag, _ffi
    c = drag_case(S, K, ragged)
    blocks = device_blocks(c, _ffi.FLAG_DRAG | (_ffi.FLAG_J2 if J2 else 0))
    chain = (*blocks, c["U"], c["units"], c["span"], C.P0_TEST, c["dens"])
    kw = dict(execution=c["ex"], q=c["q"], m_var0=c["mv"], ns=c["ns"])
    ref, refm, refb, ref_status = R.covariance_drag_chain(*chain, **kw)
    E, Em, Eb = R.chain_error_bound(*chain, **kw)
    P, Pm, Pb, status = covariance_drag(c["Y"], c["units"], c["span"], c["consts"], C.P0_TEST, c["dens"], U=c["U"], execution=c["ex"], mass_var0=c["mv"],
                                        ns=c["ns"], q=c["q"], include_J2=J2, return_status=True, return_mass=True, return_density=True)
    assert (status == 0).all() and (ref_status == 0).all()
    ratio = lambda d, r, e: (np.abs(d - r) / np.where(e > 0.0, e, 1.0)).max()
    worst = max(ratio(P, ref, E), ratio(Pm, refm, Em), ratio(Pb, refb, Eb))
    print(f"S {S} K {K} ragged {ragged} J2 {J2}: worst |device - restated| / bound = {worst:.3f}")
    assert (np.abs(P - ref) <= E).all() and (np.abs(Pm - refm) <= Em).all() and (np.abs(Pb - refb) <= Eb).all()
    assert np.array_equal(P, np.transpose(P, (0, 1, 3, 2)))
    assert np.array_equal(P[:, 0], np.broadcast_to(C.P0_TEST, (S, 6, 6))) and np.array_equal(Pm[:, 0, 6], c["mv"]) and (Pm[:, 0, :6] == 0.0).all()
    assert np.array_equal(Pb[:, 0, 7], c["dens"][:, 0] ** 2) and (Pb[:, 0, :7] == 0.0).all()
    assert (np.abs(Pb[:, 1, :3]).max(axis=1)[c["dens"][:, 0] > 0.0] > 0.0).all()           # beta reaches the position within one interval
    if c["ns"] is not None:
        for s in range(S):
            n = c["ns"][s]
            assert (P[s, n:] == 0.0).all() and (Pm[s, n:] == 0.0).all() and (Pb[s, n:] == 0.0).all() and (P[s, n - 1] != 0.0).any()


def test_same_bits():
    """A mixed batch: the satellites with sigma = 0 have conjunction.covariance_thrust's P and Pm, the others differ from it by more than
    1e-9 relative at their last node; with everything zero conjunction.covariance's P; devices=[0, 0]; a second context slot; with and
    without Pm / Pb; the _dev call over a workspace and results pre-filled with zero, big and NaN."""
    import torch
    from mpconstellation_amd import covariance, covariance_thrust, covariance_drag, conjunction as cj, _ffi
    from dev_solve import dev, filled, same_bits, _p, _stream
    S, K = 5, 30
    c = drag_case(S, K, True)
    zero = c["dens"][:, 0] == 0.0
    assert zero.tolist() == [False, True, False, False, False]
    dens = c["dens"].copy(); dens[3, 0] = 0.0; zero[3] = True
    fixed = dict(ns=c["ns"], q=c["q"], include_J2=True)
    args = (c["Y"], c["units"], c["span"], c["consts"], C.P0_TEST)
    Pt, Pmt, tst = covariance_thrust(*args, c["U"], c["ex"], mass_var0=c["mv"], include_drag=True, return_status=True, return_mass=True, **fixed)
    run = lambda **kw: covariance_drag(*args, dens, U=c["U"], execution=c["ex"], mass_var0=c["mv"], return_status=True, **fixed, **kw)
    P, Pm, Pb, st = run(return_mass=True, return_density=True)
    assert (st == 0).all() and (tst == 0).all()
    for s in range(S):
        n = c["ns"][s]
        assert (np.array_equal(P[s], Pt[s]) and np.array_equal(Pm[s], Pmt[s])) == bool(zero[s]), s
        if zero[s]:
            assert (Pb[s] == 0.0).all()
        elif n > 2:
            assert (np.abs(P[s, n - 1] - Pt[s, n - 1]) > 1e-9 * np.abs(Pt[s, n - 1])).any(), s
    # everything zero -- no execution, no mass variance, sigma = 0 -- for some satellites of a mixed batch: covariance's bits there
    plain = covariance(*args, U=c["U"], include_drag=True, **fixed)
    Pz = covariance_drag(*args, dens, U=c["U"], **fixed)
    for s in range(S):
        assert np.array_equal(Pz[s], plain[s]) == bool(zero[s]), s
    assert np.array_equal(covariance_drag(*args, [0.0, np.inf], U=c["U"], **fixed), plain)
    # alone and in the batch
    for s in (0, 4):
        one = covariance_drag(c["Y"][s:s + 1], c["units"][s:s + 1], c["span"][s:s + 1], c["consts"][s:s + 1], C.P0_TEST, dens[s:s + 1], U=c["U"][s:s + 1],
                              execution=c["ex"][s:s + 1], mass_var0=c["mv"][s:s + 1], ns=c["ns"][s:s + 1], q=c["q"][s:s + 1], include_J2=True)
        assert same_bits(one[0], P[s])
    # two contexts of one device, without Pm / Pb, another context slot
    P2, Pm2, Pb2, st2 = run(return_mass=True, return_density=True, devices=[0, 0])
    assert same_bits(P2, P) and same_bits(Pm2, Pm) and same_bits(Pb2, Pb) and same_bits(st2, st)
    P3, st3 = run()
    P4, Pb4, _ = run(return_density=True)
    assert same_bits(P3, P) and same_bits(P4, P) and same_bits(Pb4, Pb)
    flags = _ffi.FLAG_DRAG | _ffi.FLAG_J2
    out = dict(P=np.empty_like(P), Pm=np.empty_like(Pm), Pb=np.empty_like(Pb), status=np.zeros(S, dtype=np.int32))
    cj._covariance_drag_call(c["Y"], c["units"], c["span"], c["consts"], cj._check_p0(C.P0_TEST, S), c["U"], c["ns"], c["q"], _ffi.as_f64(c["ex"]), c["mv"],
                             _ffi.as_f64(dens), device=0, slot=1, out=out, flags=flags, max_step=cj.DEFAULT_MAX_STEP, atmosphere=None)
    assert same_bits(out["P"], P) and same_bits(out["Pm"], Pm) and same_bits(out["Pb"], Pb)
    # the _dev call, every device buffer a torch tensor, workspace and results pre-filled
    lib, ctx = _ffi.load(), _ffi.context(0)
    wsb = int(lib.mpcx_covariance_drag_workspace_bytes(S, K))
    assert wsb >= S * (K - 1) * _ffi.STAGE_DOUBLES * 8 and wsb % 8 == 0
    ins = [dev(a) for a in (c["ns"], c["Y"], c["U"], c["units"], c["span"], c["consts"], np.broadcast_to(C.P0_TEST, (S, 6, 6)), c["q"], c["ex"], c["mv"], dens)]
    for fill in ("zero", "big", "nan+"):
        ws, dP, dPm, dPb = filled(wsb // 8, fill), filled(S * K * 36, fill), filled(S * K * 7, fill), filled(S * K * 8, fill)
        dst = torch.full((S,), -7, dtype=torch.int32, device=ws.device)
        rc = lib.mpcx_covariance_drag_batch_dev(ctx, S, K, _p(ins[0]), _p(ins[1]), _p(ins[2]), _p(ins[3]), _p(ins[4]), _p(ins[5]), flags, cj.DEFAULT_MAX_STEP,
                                                _p(ins[6]), _p(ins[7]), _p(ins[8]), _p(ins[9]), _p(ins[10]), _p(dP), _p(dPm), _p(dPb), _p(dst), _p(ws),
                                                _stream(torch))
        _ffi.check(rc, ctx, "mpcx_covariance_drag_batch_dev")
        torch.cuda.synchronize()
        assert same_bits(dP.cpu().numpy().reshape(S, K, 6, 6), P) and same_bits(dPm.cpu().numpy().reshape(S, K, 7), Pm), fill
        assert same_bits(dPb.cpu().numpy().reshape(S, K, 8), Pb) and dst.cpu().numpy().tolist() == [0] * S, fill


def test_per_satellite_failures_leave_the_neighbours_alone():
    """every status in one call -- a count of 1 (BADK), a non-finite P0, a negative execution entry, a negative mass variance, a negative
    and a non-finite sigma, a tau of zero and a NaN tau (NUMERIC) -- each NaN in P, Pm and Pb at all K nodes; the satellites between
    them bit for bit what they are in a batch of their own (tau = inf among them); the statuses are the restatement's; an empty span
    with a bad density row is BADK"""
    from mpconstellation_amd import covariance_drag
    S, K = 11, 8
    c = drag_case(S, K, False)
    P0 = np.broadcast_to(C.P0_TEST, (S, 6, 6)).copy(); P0[2, 1, 4] = np.inf; P0[0, 5, 0] = np.nan      # (0: below the diagonal, never read)
    ex = c["ex"].copy(); ex[3, 1] = -0.1
    mv = c["mv"].copy(); mv[4] = -1e-6
    dens = c["dens"].copy(); dens[5, 0] = -0.1; dens[6, 0] = np.inf; dens[7, 1] = 0.0; dens[8, 1] = np.nan; dens[9] = (0.2, np.inf)
    ns = np.array([8, 1, 8, 8, 8, 8, 8, 8, 8, 8, 5], dtype=np.int32)
    run = lambda at: covariance_drag(c["Y"][at], c["units"][at], c["span"][at], c["consts"][at], P0[at], dens[at], U=c["U"][at], execution=ex[at],
                                     mass_var0=mv[at], ns=ns[at], q=c["q"][at], return_status=True, return_mass=True, return_density=True)
    P, Pm, Pb, st = run(np.arange(S))
    assert st.tolist() == [0, R.ST_BADK] + [R.ST_NUMERIC] * 7 + [0, 0]
    bad = st != 0
    assert np.isnan(P[bad]).all() and np.isnan(Pm[bad]).all() and np.isnan(Pb[bad]).all()
    assert np.isfinite(P[~bad]).all() and np.isfinite(Pm[~bad]).all() and np.isfinite(Pb[~bad]).all()
    good = np.array([0, 9, 10])
    Pa, Pma, Pba, sta = run(good)
    assert (sta == 0).all() and np.array_equal(Pa, P[good]) and np.array_equal(Pma, Pm[good]) and np.array_equal(Pba, Pb[good])
    z = np.zeros((S, K - 1, 7, 7)), np.zeros((S, K - 1, 7, 3)), np.zeros((S, K - 1, 7, 3)), np.zeros((S, K - 1, 7))
    *_, ref_status = R.covariance_drag_chain(*z, c["U"], c["units"], c["span"], P0, dens, execution=ex, q=c["q"], m_var0=mv, ns=ns)
    assert np.array_equal(ref_status, st)
    sp = c["span"].copy(); sp[5] = (5.0, 5.0)
    _, st = covariance_drag(c["Y"], c["units"], sp, c["consts"], C.P0_TEST, dens, U=c["U"], return_status=True)
    assert st.tolist() == [0, 0, 0, 0, 0, R.ST_BADK, R.ST_NUMERIC, R.ST_NUMERIC, R.ST_NUMERIC, 0, 0]


def test_c_abi_refusals():
    from mpconstellation_amd import _ffi
    lib, ctx = _ffi.load(), _ffi.context(0, 2)                     # (a context that never had an atmosphere)
    S, K = 2, 5
    d, i = _ffi.dptr, _ffi.iptr
    arrays = dict(X=np.ones((S, 7, K)), U=np.zeros((S, 3, K)), units=np.ones((S, 2)), span=np.array([[0.0, 1.0]] * S), consts=np.ones((S, 8)),
                  P0=np.zeros((S, 6, 6)), dens=np.zeros((S, 2)), P=np.zeros((S, K, 6, 6)))
    st = np.zeros(S, dtype=np.int32)

    def call(S=S, K=K, flags=_ffi.FLAG_DRAG, max_step=1e-2, null=None):
        p = {k: (None if k == null else d(v)) for k, v in arrays.items()}
        return lib.mpcx_covariance_drag_batch(ctx, S, K, None, p["X"], p["U"], p["units"], p["span"], p["consts"], flags, max_step, p["P0"], None,
                                              None, None, p["dens"], p["P"], None, None, None if null == "status" else i(st))
    bads = [dict(S=0), dict(K=1), dict(max_step=0.0), dict(max_step=-1.0), dict(flags=0), dict(flags=_ffi.FLAG_J2), dict(flags=_ffi.FLAG_DRAG | 4),
            dict(flags=_ffi.FLAG_DRAG | 64), dict(flags=_ffi.FLAG_DRAG | _ffi.FLAG_ATMO)] + [dict(null=k) for k in list(arrays) + ["status"]]
    for bad in bads:
        assert call(**bad) == -2, bad
        assert b"covariance_drag" in lib.mpcx_last_error(ctx), (bad, lib.mpcx_last_error(ctx))
    w = lib.mpcx_covariance_drag_workspace_bytes
    assert w(0, 5) == 0 and w(2, 1) == 0 and w(2, 5) >= 2 * 4 * _ffi.STAGE_DOUBLES * 8 and w(2, 5) == lib.mpcx_covariance_thrust_workspace_bytes(2, 5)
    assert lib.mpcx_covariance_drag_batch_dev(ctx, S, K, None, *[None] * 5, _ffi.FLAG_DRAG, 1e-2, *[None] * 11) == -2
    assert b"covariance_drag" in lib.mpcx_last_error(ctx)


# ---------------------------------------------------------------- as flown
def test_sensitivity_as_flown():
    """One satellite of the fixture's drag-scaled case with J2 (tan_K30_tf1_bigS_J2), K = 30, sigma = 1, tau = inf, P0 = 0: Pb[0, k, :6] is
    s_k = d x_k / d beta.  The same start flown by propagate_batch three times, with the constants' S times (1 + eps), (1 + eps / 2) and 1
    at eps = 0.2; r is the disagreement of the two difference quotients at the last node -- the flights' own nonlinearity and
    integrator noise, measured without the code under test.  |s_K - quotient(eps / 2)| <= 4 r + 2 x (the B_kn quadrature figure of
    test_covariance_drag_host.py) |s_K|, norms Euclidean over position / L and velocity / V.
    Measured: |s_K| 1.1600e-01, |s_K - quotient(eps / 2)| 1.311e-04, r 1.315e-04, quadrature term 2.946e-04, allowed 8.208e-04."""
    from mpconstellation_amd import covariance_drag, propagate_batch, _ffi
    from test_covariance_drag_host import QUADRATURE_FACTOR, BKN_FIGURE
    x, u, tf, cst, j2 = gold("tan_K30_tf1_bigS_J2")
    K, eps = x.shape[1], 0.2
    cs = np.repeat(cst, 3, axis=0); cs[:, C_S] *= np.array([1.0 + eps, 1.0 + eps / 2, 1.0])
    y, st, _ = propagate_batch(np.repeat(x[None, :, 0], 3, axis=0), [tf] * 3, cs, (_ffi.CTRL_SEQUENCE, np.repeat(u[None], 3, axis=0), K, 1.0), K,
                               include_drag=True, include_J2=j2)
    assert st.tolist() == [0, 0, 0]
    q_full, q_half = (y[0, :6, -1] - y[2, :6, -1]) / eps, (y[1, :6, -1] - y[2, :6, -1]) / (eps / 2)      # in L and V: normalised
    r = np.linalg.norm(q_full - q_half)
    L, Tu = float(cst[0, 6]), 5000.0
    units, span = np.array([[L, Tu]]), np.array([[0.0, tf * Tu]])
    P, Pb, status = covariance_drag(y[2:3], units, span, cst, np.zeros((6, 6)), [1.0, np.inf], U=u[None], include_J2=j2, return_status=True,
                                    return_density=True)
    assert status.tolist() == [0]
    s = Pb[0, -1, :6] / np.array([L] * 3 + [L / Tu] * 3)
    err, quad = np.linalg.norm(s - q_half), QUADRATURE_FACTOR * BKN_FIGURE["tan_K30_tf1_bigS_J2"] * np.linalg.norm(s)
    print(f"as flown: |s_K| {np.linalg.norm(s):.4e}, |s_K - quotient(eps/2)| {err:.3e}, flights' own disagreement r {r:.3e}, quadrature term {quad:.3e}; "
          f"allowed {4 * r + quad:.3e}")
    assert np.linalg.norm(s) > 100.0 * r and err <= 4.0 * r + quad
    assert np.array_equal(Pb[0, :, 7], np.ones(K)) and np.abs(P[0, -1] - np.outer(Pb[0, -1, :6], Pb[0, -1, :6])).max() <= 1e-9 * np.abs(P[0, -1]).max()


# ---------------------------------------------------------------- end to end
def test_end_to_end_a_density_error_widens_the_planted_encounter():
    """The planted scene of test_covariance_thrust_gpu.py's last test on drag-scaled constants (ARC_S_SCALE) with drag in the model: the arc flown by
    propagate_batch(include_drag=True), an object planted 200 m away in the encounter plane, screen_against, then collision_probability
    twice on the same screen: with covariance_thrust's P (2 %, 1 degree) and with covariance_drag's at sigma = 0.2, tau = inf on top.
    The frame is the same (miss and relative speed to the bit); the Mahalanobis distance with the density error is strictly smaller;
    P_drag - P_thrust is positive semidefinite at every node to the two chains' bounds.  ConstellationMPC.plan_covariance(density=...)
    is the direct call bit for bit and raises with plan_drag=False.  Measured: miss 199.75 m; 1.340000 sigma, Pc 1.932e-04, sigmas
    (744.8, 141.6) m with execution errors alone; 0.516536 sigma, Pc 1.761e-05, sigmas (8323.7, 298.6) m with the density bias."""
    from mpconstellation_amd import screen_against, covariance, covariance_thrust, covariance_drag, collision_probability, propagate_batch, _ffi
    from test_avoidance_gpu import scale_constants
    a = AR.arc_setup()
    K = AR.SCENE["K"]
    consts = a["consts"][None].copy(); consts[:, C_S] *= ARC_S_SCALE
    y, st, _ = propagate_batch(a["y0"][None], [AR.SCENE["tf"]], consts, (_ffi.CTRL_SEQUENCE, a["U"][None], K, 1.0), K, include_drag=True,
                               max_step=AR.SCENE["prop_max_step"])
    assert st.tolist() == [0]
    x = y[0]
    hn = (a["span"][1] - a["span"][0]) / (K - 1)
    cy, cu, cspan = AR.planted_object(dict(a, x=x), a["span"][0] + 20.37 * hn)
    units, span = a["units"][None], a["span"][None]
    cY, cunits, cspans = cy[None], cu[None], cspan[None]
    P0 = np.diag([40.0 ** 2] * 3 + [0.02 ** 2] * 3)
    cP = covariance(cY, cunits, cspans, scale_constants(cunits[:, 0]), P0)
    scr = screen_against(Y=x[None], units=units, span=span, cat_Y=cY, cat_units=cunits, cat_span=cspans, M=4 * (K - 1) + 1, T0=float(span[0, 0]),
                         T1=float(span[0, 1]), threshold=5000.0)
    ex, dens = np.array([0.0, 0.02, 0.0, 0.01745, 0.0]), np.array([0.2, np.inf])
    P_t, st_t = covariance_thrust(x[None], units, span, consts, P0, a["U"][None], ex, include_drag=True, return_status=True)
    P_d, st_d = covariance_drag(x[None], units, span, consts, P0, dens, U=a["U"][None], execution=ex, return_status=True)
    prob = lambda P: collision_probability(scr, 5.0, x[None], units, span, P, cat=(cY, cunits, cspans, cP, 5.0))
    col_t, col_d = prob(P_t), prob(P_d)
    print(f"planted encounter: miss {col_t.miss[0]:.2f} m; execution errors alone {col_t.mahalanobis[0]:.6f} sigma, Pc {col_t.pc[0]:.3e}, sigma "
          f"{col_t.sigma[0]} m; with a 20 % density bias {col_d.mahalanobis[0]:.6f} sigma, Pc {col_d.pc[0]:.3e}, sigma {col_d.sigma[0]} m")
    assert st_t.tolist() == [0] and st_d.tolist() == [0] and col_t.status.tolist() == [0] and col_d.status.tolist() == [0]
    assert col_t.miss[0] == col_d.miss[0] and col_t.speed[0] == col_d.speed[0]
    assert col_d.mahalanobis[0] < col_t.mahalanobis[0]
    c = dict(Y=x[None], U=a["U"][None], units=units, span=span, consts=consts, ns=None)
    A, Bn, Bp, G = device_blocks(c, _ffi.FLAG_DRAG)
    Ed, _, _ = R.chain_error_bound(A, Bn, Bp, G, a["U"][None], units, span, P0, dens, execution=ex)
    Et, _ = T.chain_error_bound(A, Bn, Bp, a["U"][None], units, span, P0, ex)
    for k in range(K):
        w = np.linalg.eigvalsh(P_d[0, k] - P_t[0, k])
        assert w.min() >= -(np.linalg.norm(Ed[0, k]) + np.linalg.norm(Et[0, k])), (k, w)
    assert np.array_equal(P_d[0, 0], P_t[0, 0]) and np.linalg.eigvalsh(P_d[0, -1] - P_t[0, -1]).max() > 0.0
    # through ConstellationMPC: the plan put in by hand (test_avoidance_joint_gpu.arc_instance), drag in the planning model
    from test_avoidance_joint_gpu import arc_instance
    mpc, _ = arc_instance()
    mpc.consts = mpc.consts.copy(); mpc.consts[:, C_S] *= ARC_S_SCALE
    with pytest.raises(ValueError, match="density"):
        mpc.plan_covariance(P0, density=dens)
    with pytest.raises(ValueError, match="density"):
        mpc.collision_probability(5000.0, P0, 5.0, density=dens)
    mpc.plan_drag = True
    (w,) = mpc._screen_windows("plan", 1)
    direct = covariance_drag(w["Y"], w["units"], w["span"], mpc.consts, P0, dens, U=mpc._plan[1], execution=ex, ns=w["ns"], include_J2=mpc.plan_J2,
                             atmosphere=mpc.atmosphere)
    assert np.array_equal(mpc.plan_covariance(P0, execution=ex, density=dens), direct) and np.isfinite(direct).all()
    assert not np.array_equal(mpc.plan_covariance(P0, execution=ex), direct)
