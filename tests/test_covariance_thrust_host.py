"""The covariance chain with thrust execution errors without a GPU: the restatement (covariance_thrust_reference.py, the formulas of
include/mpcx.h: mpcx_covariance_thrust_batch) against an independent truth from the CPU oracle's nonlinear flow, its zero case against
collision_reference.covariance_chain, statuses, gates_execution, and the wrappers' marshalling and validation with a recorder in
place of the library.

The truth.  On covariance_thrust_reference.eccentric_arc(K) -- a thrusting arc from the perigee of an e = 0.1 orbit, propagated and
linearised by the oracle -- G_k,m = d x_k / d u_m and Phi_k,0 = d x_k / d x_0 come from central differences of the nonlinear flow, and
P_k = Phi_k,0 P_0 Phi_k,0^T + sum_m G_k,m Sigma_m G_k,m^T.  The restatement's chain on the oracle's A, B_kn, B_kp differs from it by
the linearisation's own error (the discretiser's rtol 1e-3 quadrature; mpcx_avoidance's sensitivities measure 2.4e-3 .. 3.5e-3 on
such records).  Measure: per node, the worst entry error over the largest entry of the node's 6 x 6 truth, both in the orbit's own
units (lengths over L, velocities over L / Tu: every block counts alike), the maximum over the nodes; the mass row -- the mass's
covariances with position and velocity in the same units, and the mass variance -- is measured the same way on its own, because
in those units the mass variance is eight orders of magnitude above every other entry of the 7 x 7."""
import numpy as np
import pytest

import collision_reference as C
import covariance_thrust_reference as T

# execution errors of the truth check: fixed 1e-4 and 2 % in magnitude, fixed 1e-4 and 1 degree in pointing, off below 1e-3
EXEC = np.array([1e-4, 0.02, 1e-4, 0.01745, 1e-3])
P0_SMALL = 1e-2 * C.P0_TEST                    # sigmas of 5 .. 30 m: the thrust errors dominate the later nodes
M_VAR0 = 0.01 ** 2                             # a 1 % mass sigma at the first node
# Measured when this file was written (test_restatement_against_the_nonlinear_truth prints them): the measure above, per case.
# The mutated chains measure: without the cross term 2.6e-1 (K = 8) and 3.2e-1 (K = 30), B_kn / B_kp swapped 1.1e-1 and 9.4e-3,
# without the mass row and column (m_var0 > 0) 9.6e-2 and 2.4e-1.
TRUTH_MEASURED = {(8, "exec"): 5.833e-4, (30, "exec"): 2.078e-4, (8, "mass"): 5.642e-4, (30, "mass"): 8.674e-5,
                  (8, "mass row"): 4.119e-6, (30, "mass row"): 7.105e-6}
TRUTH_BOUND = {k: 3.0 * v for k, v in TRUTH_MEASURED.items()}


def seven(P, Pm):
    """(K, 7, 7) from the position / velocity block and the mass row"""
    K = P.shape[0]
    out = np.zeros((K, 7, 7))
    out[:, :6, :6] = P
    out[:, 6, :] = Pm
    out[:, :, 6] = Pm
    return out


def mismatch(P7, truth, units):
    """the measure on the position / velocity block"""
    L, Tu = units
    d = 1.0 / np.array([L] * 3 + [L / Tu] * 3)
    a, b = P7[:, :6, :6] * d[:, None] * d[None, :], truth[:, :6, :6] * d[:, None] * d[None, :]
    return max(np.abs(a[k] - b[k]).max() / np.abs(b[k]).max() for k in range(1, len(b)))


def mismatch_mass(P7, truth, units):
    """the measure on the mass's covariances with position and velocity, and the relative error of the mass variance"""
    L, Tu = units
    d = 1.0 / np.array([L] * 3 + [L / Tu] * 3)
    a, b = P7[:, 6, :6] * d, truth[:, 6, :6] * d
    return max(max(np.abs(a[k] - b[k]).max() / np.abs(b[k]).max(), abs(P7[k, 6, 6] - truth[k, 6, 6]) / truth[k, 6, 6]) for k in range(1, len(b)))


def restated(K, m_var0=None, **mutation):
    sc = T.eccentric_arc(K)
    P, Pm, st = T.covariance_thrust_chain(sc["A"][None], sc["Bn"][None], sc["Bp"][None], sc["U"][None], sc["units"][None], sc["span"][None],
                                          P0_SMALL, EXEC, m_var0=m_var0, **mutation)
    assert st.tolist() == [0]
    return seven(P[0], Pm[0])


@pytest.mark.parametrize("K", [8, 30])
def test_restatement_against_the_nonlinear_truth(K):
    """The restated chain within 3 x the measured mismatch of the finite-difference truth, with proportional and fixed terms and two
    nodes off; under the same assertion the chain without the cross term Y + Y^T and the chain with B_kn and B_kp swapped fail; and
    with a mass variance at the first node, the chain without the mass row and column fails."""
    sc = T.eccentric_arc(K)
    assert (sc["U"][:, 2] == 0.0).all() and (sc["U"][:, -1] == 0.0).all()
    truth = T.truth_covariance(K, P0_SMALL, EXEC)
    good = mismatch(restated(K), truth, sc["units"])
    no_cross = mismatch(restated(K, cross=False), truth, sc["units"])
    swapped = mismatch(restated(K, swap=True), truth, sc["units"])
    print(f"K {K}: mismatch {good:.3e} (bound {TRUTH_BOUND[K, 'exec']:.3e}); without the cross term {no_cross:.3e}, B_kn / B_kp swapped {swapped:.3e}")
    truth_m = T.truth_covariance(K, P0_SMALL, EXEC, M_VAR0)
    good_m, row_m = mismatch(restated(K, M_VAR0), truth_m, sc["units"]), mismatch_mass(restated(K, M_VAR0), truth_m, sc["units"])
    no_mass = mismatch(restated(K, M_VAR0, mass=False), truth_m, sc["units"])
    print(f"K {K}, mass variance: mismatch {good_m:.3e} (bound {TRUTH_BOUND[K, 'mass']:.3e}), mass row {row_m:.3e} (bound "
          f"{TRUTH_BOUND[K, 'mass row']:.3e}); without the mass row and column {no_mass:.3e}")
    assert good <= TRUTH_BOUND[K, "exec"] and good_m <= TRUTH_BOUND[K, "mass"] and row_m <= TRUTH_BOUND[K, "mass row"]
    assert no_cross > TRUTH_BOUND[K, "exec"] and swapped > TRUTH_BOUND[K, "exec"]
    assert no_mass > TRUTH_BOUND[K, "mass"]


def test_zero_execution_is_the_plain_chain_and_the_difference_is_positive_semidefinite():
    sc = T.eccentric_arc(30)
    args = (sc["units"][None], sc["span"][None], C.P0_TEST)
    plain, st = C.covariance_chain(sc["A"][None], *args, q=1e-7)
    P, Pm, st2 = T.covariance_thrust_chain(sc["A"][None], sc["Bn"][None], sc["Bp"][None], sc["U"][None], *args, np.zeros(5), q=1e-7)
    assert st.tolist() == st2.tolist() == [0]
    assert np.array_equal(P, plain) and (Pm == 0.0).all()
    Pt, Pmt, _ = T.covariance_thrust_chain(sc["A"][None], sc["Bn"][None], sc["Bp"][None], sc["U"][None], *args, EXEC, q=1e-7, m_var0=M_VAR0)
    assert np.array_equal(Pt, np.transpose(Pt, (0, 1, 3, 2))) and np.array_equal(Pt[0, 0], C.P0_TEST) and Pmt[0, 0].tolist() == [0.0] * 6 + [M_VAR0]
    L, Tu = sc["units"]
    d = 1.0 / np.array([L] * 3 + [L / Tu] * 3)
    for k in range(1, 30):
        diff = (Pt[0, k] - plain[0, k]) * d[:, None] * d[None, :]
        w = np.linalg.eigvalsh(diff)
        assert w.max() > 0.0 and w.min() >= -1e-10 * w.max(), (k, w)
    assert (Pmt[0, 1:, 6] > 0.0).all()


def test_statuses():
    sc = T.eccentric_arc(8)
    S = 7
    rep = lambda a: np.repeat(np.asarray(a)[None], S, axis=0)
    P0 = rep(C.P0_TEST).copy(); P0[2, 1, 4] = np.inf
    ex = rep(EXEC).copy(); ex[3, 1] = -0.1; ex[4, 4] = np.nan
    mv = np.zeros(S); mv[5] = -1e-6
    ns = np.array([8, 1, 8, 8, 8, 8, 5], dtype=np.int32)
    P, Pm, st = T.covariance_thrust_chain(rep(sc["A"]), rep(sc["Bn"]), rep(sc["Bp"]), rep(sc["U"]), rep(sc["units"]), rep(sc["span"]), P0, ex,
                                          m_var0=mv, ns=ns)
    assert st.tolist() == [0, T.ST_BADK, T.ST_NUMERIC, T.ST_NUMERIC, T.ST_NUMERIC, T.ST_NUMERIC, 0]
    bad = st != 0
    assert np.isnan(P[bad]).all() and np.isnan(Pm[bad]).all() and np.isfinite(P[~bad]).all() and np.isfinite(Pm[~bad]).all()
    assert (P[6, 5:] == 0.0).all() and (Pm[6, 5:] == 0.0).all() and (P[6, 4] != 0.0).any()
    _, _, st = T.covariance_thrust_chain(rep(sc["A"]), rep(sc["Bn"]), rep(sc["Bp"]), rep(sc["U"]), rep(sc["units"]), rep(sc["span"]), P0, ex,
                                         m_var0=mv, ns=ns, disc_status=np.array([0, 2, 3, 0, 0, 0, 0]))
    assert st.tolist() == [0, T.ST_BADK, 3, T.ST_NUMERIC, T.ST_NUMERIC, T.ST_NUMERIC, 0]          # covariance's statuses first, in its order


def test_gates_execution_against_hand_values():
    from mpconstellation_amd import gates_execution, conjunction as cj
    from mpconstellation_amd.satellite_scale import SatelliteScale
    scales = [SatelliteScale(x=np.array([7.0e6, 0.0, 0.0, 0.0, 7.5e3, 0.0, 100.0])), SatelliteScale(x=np.array([7.4e6, 0.0, 0.0, 0.0, 7.3e3, 0.0, 250.0]))]
    f = [sc.units["force"] for sc in scales]
    ex = gates_execution(scales, fixed_magnitude_N=1e-3, proportional_magnitude=0.02, fixed_pointing_N=[2e-3, 4e-3], proportional_pointing_rad=0.01745,
                         off_N=5e-3)
    assert ex.shape == (2, 5) and ex.flags.c_contiguous
    assert ex.tolist() == [[1e-3 / f[0], 0.02, 2e-3 / f[0], 0.01745, 5e-3 / f[0]], [1e-3 / f[1], 0.02, 4e-3 / f[1], 0.01745, 5e-3 / f[1]]]
    assert (gates_execution(scales) == 0.0).all()
    assert f[0] != f[1] and f[0] == scales[0].units["mass"] * scales[0].units["length"] / scales[0].units["time"] ** 2
    for kw in (dict(fixed_magnitude_N=-1.0), dict(proportional_magnitude=np.nan), dict(off_N=[1.0, 2.0, 3.0]), dict(fixed_pointing_N=np.ones((2, 1)))):
        with pytest.raises(ValueError):
            gates_execution(scales, **kw)
    assert cj.gates_execution is gates_execution


S, N = 4, 6
GOOD = dict(Y=np.zeros((S, 7, N)), units=np.ones((S, 2)), span=np.array([[0.0, 1.0]] * S), consts=np.ones((S, 8)), P0=np.eye(6),
            U=np.ones((S, 3, N)), execution=EXEC)


def test_wrapper_argument_checks(monkeypatch):
    from mpconstellation_amd import conjunction as cj, _ffi

    def no_call(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_ffi, "call", no_call)
    monkeypatch.setattr(_ffi, "context", no_call)
    bad = [dict(U=None), dict(U=np.ones((S, 3, N + 1))), dict(execution=np.zeros(4)), dict(execution=np.zeros((S + 1, 5))), dict(execution=np.zeros((S, 6))),
           dict(mass_var0=[1.0, 2.0]), dict(mass_var0=np.ones((S, 1))), dict(P0=np.eye(5)), dict(q=-1.0), dict(q=[1.0, 2.0]), dict(consts=np.ones((S, 7))),
           dict(Y=np.zeros((S, 7, 1)), U=np.ones((S, 3, 1))), dict(max_step=0.0), dict(ns=[5]), dict(units=np.ones((S, 3)))]
    for kw in bad:
        with pytest.raises(ValueError):
            cj.covariance_thrust(**{**GOOD, **kw})
    with pytest.raises(ValueError, match=r"execution.*\(5,\) or \(4, 5\)"):
        cj.covariance_thrust(**{**GOOD, "execution": np.zeros((5, 4))})
    with pytest.raises(AssertionError, match="the library was called"):
        cj.covariance_thrust(**GOOD)


class Recorder:
    """stands in for _ffi.call: keeps every call's name and arguments, fills P with the block's first satellite index"""

    def __init__(self):
        self.calls = []

    def __call__(self, name, ctx, *args):
        self.calls.append((name, ctx, args))


def addr(p):
    import ctypes
    return None if p is None else ctypes.cast(p, ctypes.c_void_p).value


def test_wrapper_marshalling(monkeypatch):
    from mpconstellation_amd import conjunction as cj, _ffi
    rec = Recorder()
    monkeypatch.setattr(_ffi, "call", rec)
    monkeypatch.setattr(_ffi, "context", lambda device=0, slot=0: (device, slot))
    ex = np.arange(S * 5, dtype=np.float64).reshape(S, 5)
    U = np.arange(S * 3 * N, dtype=np.float64).reshape(S, 3, N)
    out = cj.covariance_thrust(**{**GOOD, "U": U, "execution": ex, "include_J2": True, "max_step": 0.125})
    assert isinstance(out, np.ndarray) and out.shape == (S, N, 6, 6)
    (name, ctx, a), = rec.calls
    assert name == "mpcx_covariance_thrust_batch" and ctx == (0, 0) and len(a) == 17
    # S, K, Ks, X, U, units, span, consts, flags, max_step, P0, q, exec, m_var0, P, Pm, status
    assert a[0] == S and a[1] == N and a[2] is None and a[8] == _ffi.FLAG_J2 and a[9] == 0.125
    assert a[11] is None and a[13] is None and a[15] is None                       # q, m_var0, Pm: NULL
    assert addr(a[4]) == U.ctypes.data and addr(a[12]) == ex.ctypes.data and addr(a[14]) == out.ctypes.data
    assert np.ctypeslib.as_array(a[10], shape=(S, 6, 6)).tolist() == [np.eye(6).tolist()] * S          # a (6, 6) P0 is broadcast
    # a (5,) execution is broadcast; mass_var0, q, ns, Pm and status are passed; the results come as P, Pm, status
    rec.calls.clear()
    P, Pm, st = cj.covariance_thrust(**{**GOOD, "mass_var0": 2.5, "q": 1e-6, "ns": [6, 5, 4, 3]}, return_mass=True, return_status=True, device=3)
    (name, ctx, a), = rec.calls
    assert ctx == (3, 0) and Pm.shape == (S, N, 7) and st.shape == (S,) and st.dtype == np.int32
    assert np.ctypeslib.as_array(a[12], shape=(S, 5)).tolist() == [EXEC.tolist()] * S
    assert np.ctypeslib.as_array(a[13], shape=(S,)).tolist() == [2.5] * S and np.ctypeslib.as_array(a[11], shape=(S,)).tolist() == [1e-6] * S
    assert np.ctypeslib.as_array(a[2], shape=(S,)).tolist() == [6, 5, 4, 3]
    assert addr(a[14]) == P.ctypes.data and addr(a[15]) == Pm.ctypes.data and addr(a[16]) == st.ctypes.data
    assert len(cj.covariance_thrust(**GOOD, return_status=True)) == 2 and len(cj.covariance_thrust(**GOOD, return_mass=True)) == 2
    # devices=[0, 0]: two contiguous blocks on two contexts of device 0, each writing its own part of ONE result set
    rec.calls.clear()
    P, Pm, st = cj.covariance_thrust(**{**GOOD, "U": U, "execution": ex, "mass_var0": np.arange(S) + 1.0}, devices=[0, 0], return_mass=True,
                                     return_status=True)
    calls = sorted(rec.calls, key=lambda c: c[1])
    assert [c[1] for c in calls] == [(0, 0), (0, 1)] and [c[2][0] for c in calls] == [2, 2]
    for b, (_, _, a) in enumerate(calls):
        assert addr(a[4]) == U[2 * b:].ctypes.data and addr(a[12]) == ex[2 * b:].ctypes.data
        assert np.ctypeslib.as_array(a[13], shape=(2,)).tolist() == [2 * b + 1.0, 2 * b + 2.0]
        assert addr(a[14]) == P[2 * b:].ctypes.data and addr(a[15]) == Pm[2 * b:].ctypes.data and addr(a[16]) == st[2 * b:].ctypes.data
    rec.calls.clear()
    cj.covariance_thrust(**GOOD, devices=[2])
    assert [c[1] for c in rec.calls] == [(2, 0)]


def planned_mpc():
    """test_conjunction_host's hand-made constellation with a plan put in by hand"""
    from test_conjunction_host import hand_made_mpc
    mpc, _ = hand_made_mpc()
    rng = np.random.default_rng(1)
    mpc._plan = (rng.normal(size=(3, 7, 5)), rng.normal(size=(3, 3, 5)), np.zeros((3, 7, 4)))
    mpc.plan_K, mpc.plan_tf = np.array([5, 5, 4]), np.array([0.5, 0.5, 0.4])
    return mpc


def test_constellation_mpc_calls(monkeypatch):
    """with the defaults plan_covariance, collision_probability and collision_probability_window make the library calls they made
    before (mpcx_covariance_batch with the same arguments as conjunction.covariance on the plan); with execution they call
    mpcx_covariance_thrust_batch with the plan's thrust, the planning model's flags and the execution rows"""
    from mpconstellation_amd import conjunction as cj, _ffi
    rec = Recorder()
    monkeypatch.setattr(_ffi, "call", rec)
    monkeypatch.setattr(_ffi, "context", lambda device=0, slot=0: (device, slot))
    mpc = planned_mpc()
    (w,) = mpc._screen_windows("plan", 4)
    cj.covariance(w["Y"], w["units"], w["span"], mpc.consts, np.eye(6), U=mpc._plan[1], ns=w["ns"], q=1e-8)
    (want,) = rec.calls
    values = lambda a: [x if isinstance(x, (int, float, type(None))) else None for x in a]
    for run in (lambda **kw: mpc.plan_covariance(np.eye(6), q=1e-8, **kw), lambda **kw: mpc.collision_probability(1000.0, np.eye(6), 5.0, q=1e-8, **kw),
                lambda **kw: mpc.collision_probability_window(1000.0, np.eye(6), 5.0, 60.0, q=1e-8, **kw)):
        rec.calls.clear()
        run()
        names = [c[0] for c in rec.calls]
        assert names.count("mpcx_covariance_batch") == 1 and "mpcx_covariance_thrust_batch" not in names
        got = rec.calls[names.index("mpcx_covariance_batch")]
        assert values(got[2]) == values(want[2]) and addr(got[2][4]) == mpc._plan[1].ctypes.data
        rec.calls.clear()
        run(execution=EXEC, mass_var0=1e-4)
        names = [c[0] for c in rec.calls]
        assert names.count("mpcx_covariance_thrust_batch") == 1 and "mpcx_covariance_batch" not in names
        a = rec.calls[names.index("mpcx_covariance_thrust_batch")][2]
        assert a[0] == 3 and a[1] == 5 and addr(a[4]) == mpc._plan[1].ctypes.data and a[8] == 0
        assert np.ctypeslib.as_array(a[2], shape=(3,)).tolist() == [5, 5, 4]
        assert np.ctypeslib.as_array(a[12], shape=(3, 5)).tolist() == [EXEC.tolist()] * 3 and np.ctypeslib.as_array(a[13], shape=(3,)).tolist() == [1e-4] * 3
    with pytest.raises(ValueError, match="mass_var0"):
        mpc.plan_covariance(np.eye(6), mass_var0=1e-4)
    from test_conjunction_host import hand_made_mpc
    with pytest.raises(ValueError, match="no plan"):
        hand_made_mpc()[0].plan_covariance(np.eye(6))


def test_names_are_exported():
    import mpconstellation_amd as pkg
    from mpconstellation_amd import _ffi
    assert {"covariance_thrust", "gates_execution"} <= set(pkg.__all__) and callable(pkg.covariance_thrust) and callable(pkg.gates_execution)
    assert {"mpcx_covariance_thrust_workspace_bytes", "mpcx_covariance_thrust_batch", "mpcx_covariance_thrust_batch_dev"} <= set(_ffi.exported_symbols())
    assert _ffi.NEXEC == 5 and hasattr(pkg.ConstellationMPC, "plan_covariance")
