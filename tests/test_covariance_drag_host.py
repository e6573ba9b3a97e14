"""The covariance chain with an uncertain drag without a GPU: the drag column of the stage records as covariance_drag_reference.py
forms it from the CPU oracle's quadrature nodes against an independent integration of the variational equation, and identities of the
restated chain (include/mpcx.h: mpcx_covariance_drag_batch).

The column.  G_k = d x_k+1 / d beta solves s' = (tf Dxf) s + tf [0; a_D; 0], s(tau_k) = 0, along the interval's own nonlinear flow.
scipy's DOP853 at rtol 1e-12 integrates (x, s, b) through oracle_lib.dynamics and oracle_lib.A_func, b the same equation with the
forcing B_func[:, 0] lambda^-(tau): b(tau_k+1) is the first column of B_kn, which the same record holds, from the same nodes by the same
trapezoid.  The quadrature's own error is what separates either column from its integration (the RK45 nodes at rtol 1e-3 are few),
so the tolerance is relative: relerr(G) <= 2 relerr(B_kn[:, 0]) -- the forcing of G is about as smooth as that of B_kn.
Measured when this file was written (relerr over all intervals; the test prints them):
    tan_K30_tf1              G 5.571e-04   B_kn column 1.262e-03   (ratio 0.44)
    tan_K30_tf1_bigS_J2      G 5.571e-04   B_kn column 1.265e-03   (ratio 0.44)
    atmosphere (350 x 420 km, `general`, J2, K 12, tf 1.5)   G 1.841e-03   B_kn column 3.303e-03   (ratio 0.56)
"""
import functools
import os

import numpy as np
import pytest

import collision_reference as C
import covariance_drag_reference as R
import covariance_thrust_reference as T
import oracle_lib as O

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "drag_discretize.npz"))
QUADRATURE_FACTOR = 2.0          # relerr(G) <= this times relerr(B_kn's first column); test_covariance_drag_gpu.py's flown check reads it
# the B_kn figures above, rounded up: the test holds the measured ones to them, and the flown check on the device takes the quadrature's
# share of its tolerance from here
BKN_FIGURE = {"tan_K30_tf1": 1.27e-3, "tan_K30_tf1_bigS_J2": 1.27e-3, "atmosphere": 3.31e-3}
EXEC = np.array([1e-4, 0.02, 1e-4, 0.01745, 1e-3])


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def column_case(name):
    """-> (x (7, K), u (3, K), tf, const, oracle flags, atmosphere)"""
    if name == "atmosphere":
        import drag_cases as D
        b = D.batch()
        return b["x"][1], b["u"][1], float(b["tf"][1]), b["const"][1], O.FLAG_DRAG | O.FLAG_J2, D.models()["general"]
    g = lambda k: GOLD[f"{k}_{name}"]
    return g("x"), g("u"), float(g("tf")), g("const"), O.FLAG_DRAG | (O.FLAG_J2 if bool(g("j2")) else 0), None


@functools.lru_cache(maxsize=None)
def integrated_columns(name):
    """(G, B_kn[:, 0]) (K-1, 7) each by DOP853 at rtol 1e-12 over every node interval, from the interval's own first node"""
    from scipy.integrate import solve_ivp
    x, u, tf, cst, flags, atm = column_case(name)
    K = x.shape[1]
    tau = np.linspace(0.0, 1.0, K)
    G, B0 = np.zeros((K - 1, 7)), np.zeros((K - 1, 7))
    for k in range(K - 1):
        def rhs(t, z):
            y, s, b = z[:7], z[7:14], z[14:]
            ut, rc = O.u_foh(t, u)
            f, rc2 = O.dynamics(y, ut, tf, cst, flags, atm)
            assert rc == 0 and rc2 == 0
            A = O.A_func(y, ut, tf, cst, flags, atm)
            lam_n = (tau[k + 1] - t) / (tau[k + 1] - tau[k])
            return np.concatenate([f, A @ s + R.drag_forcing(y, tf, cst, flags, atm), A @ b + O.B_func(y, ut, tf, cst)[:, 0] * lam_n])
        sol = solve_ivp(rhs, (tau[k], tau[k + 1]), np.concatenate([x[:, k], np.zeros(14)]), method="DOP853", rtol=1e-12, atol=1e-15)
        assert sol.success
        G[k], B0[k] = sol.y[7:14, -1], sol.y[14:, -1]
    return G, B0


@pytest.mark.parametrize("name", ["tan_K30_tf1", "tan_K30_tf1_bigS_J2", "atmosphere"])
def test_drag_column_against_an_independent_integration(name):
    x, u, tf, cst, flags, atm = column_case(name)
    G, d = R.drag_column(x, u, tf, cst, flags, atm)
    Gi, Bi = integrated_columns(name)
    eg, eb = relerr(G, Gi), relerr(d["Bn"][:, :, 0], Bi)
    print(f"{name}: relerr of the drag column {eg:.3e}, of B_kn's first column {eb:.3e} (ratio {eg / eb:.2f}, allowed {QUADRATURE_FACTOR})")
    assert (G[:, 6] == 0.0).all() and np.abs(G[:, :6]).max() > 0.0                   # the mass row is zero, the column is not
    assert eg <= QUADRATURE_FACTOR * eb and eb <= BKN_FIGURE[name]
    # the forcing itself: taking the difference with gravity and thrust in place agrees with the one drag_forcing takes to the
    # cancellation it was written to avoid (an acceleration of order 1 in these units: a few ulp of 1)
    y = x[:, 3]
    f1, _ = O.dynamics(y, u[:, 3], tf, cst, flags, atm)
    f0, _ = O.dynamics(y, u[:, 3], tf, cst, flags & ~O.FLAG_DRAG)
    assert np.abs((f1 - f0) - R.drag_forcing(y, tf, cst, flags, atm)).max() <= 16 * np.finfo(float).eps * tf * max(np.abs(f1).max(), 1.0)


@functools.lru_cache(maxsize=None)
def chain_inputs():
    """the records of the drag-scaled golden case with its drag column, in physical units of a Hubble-like orbit; P0 and the rest"""
    x, u, tf, cst, flags, atm = column_case("tan_K30_tf1_bigS_J2")
    G, d = R.drag_column(x, u, tf, cst, flags, atm)
    L, Tu = float(cst[6]), 900.0
    units, span = np.array([[L, Tu]]), np.array([[0.0, tf * Tu]])
    return dict(A=d["A"][None], Bn=d["Bn"][None], Bp=d["Bp"][None], G=G[None], U=u[None], units=units, span=span, K=x.shape[1])


def _chain(c, density, **kw):
    return R.covariance_drag_chain(c["A"], c["Bn"], c["Bp"], c["G"], c["U"], c["units"], c["span"], C.P0_TEST, density, **kw)


def test_a_bias_adds_sigma_squared_s_s_transpose():
    """tau = inf: P - P_thrust_chain = sigma^2 s s^T with s_k+1 = Phi~ s_k + G~, inside the two chains' bounds; Pb[:, :6] = sigma^2 s_k"""
    c = chain_inputs()
    sig = 0.2
    kw = dict(execution=EXEC, q=1e-7, m_var0=1e-4)
    P, Pm, Pb, st = _chain(c, [sig, np.inf], **kw)
    Pt, Pmt, stt = T.covariance_thrust_chain(c["A"], c["Bn"], c["Bp"], c["U"], c["units"], c["span"], C.P0_TEST, EXEC, q=1e-7, m_var0=1e-4)
    E, Em, Eb = R.chain_error_bound(c["A"], c["Bn"], c["Bp"], c["G"], c["U"], c["units"], c["span"], C.P0_TEST, [sig, np.inf], **kw)
    Et, Emt = T.chain_error_bound(c["A"], c["Bn"], c["Bp"], c["U"], c["units"], c["span"], C.P0_TEST, EXEC, q=1e-7, m_var0=1e-4)
    assert st.tolist() == [0] and stt.tolist() == [0]
    L, Tu = c["units"][0]
    s = np.zeros(7)
    for k in range(c["K"] - 1):
        p8 = R.phi8(c["A"][0, k], c["G"][0, k], L, Tu, 1.0)
        s = p8[:7, :7] @ s + p8[:7, 7]
        add = sig * sig * np.outer(s, s)
        assert (np.abs((P[0, k + 1] - Pt[0, k + 1]) - add[:6, :6]) <= E[0, k + 1] + Et[0, k + 1]).all(), k
        assert (np.abs((Pm[0, k + 1] - Pmt[0, k + 1]) - add[6]) <= Em[0, k + 1] + Emt[0, k + 1]).all(), k
        assert (np.abs(Pb[0, k + 1, :7] - sig * sig * s) <= Eb[0, k + 1, :7]).all(), k
        assert Pb[0, k + 1, 7] == sig * sig
    assert np.abs(P[0, -1] - Pt[0, -1]).max() > 1e3 * (E[0, -1] + Et[0, -1]).max()       # (the identity is about something)


def test_the_variance_of_beta_is_stationary():
    """Var beta_k = sigma^2 at every node for a finite tau, to a few ulp: v' = phi (phi v) + (1 - phi^2) sigma^2.  With u = eps / 2 the
    unit roundoff and v ~ sigma^2, a step adds, relative to sigma^2: u phi (the inner product, of size phi sigma^2), u phi^2 (the outer
    one), u (the sum) and 3 u (1 - phi^2) (the noise: phi^2, 1 - phi^2 and the product by sigma^2, each relative to the noise's own
    size) -- u (4 + phi - 2 phi^2) <= 4.125 u = 2.0625 eps, largest at phi = 1 / 4 -- and passes the error it was given on times phi^2 <= 1.  Node k is within 2.25 k eps of sigma^2 whatever tau (2.0625 and
    the second-order terms).  (Measured: 0 for tau << h, 20 eps at node 29 for tau = 1e9 h.)"""
    c = chain_inputs()
    h = (c["span"][0, 1] - c["span"][0, 0]) / (c["K"] - 1)
    for tau in (0.01 * h, h, 40.0 * h, 1e9 * h):
        _, _, Pb, st = _chain(c, [0.3, tau], q=1e-7)
        assert st.tolist() == [0]
        assert Pb[0, 0, 7] == 0.3 * 0.3
        assert (np.abs(Pb[0, :, 7] / Pb[0, 0, 7] - 1.0) <= 2.25 * np.arange(c["K"]) * np.finfo(float).eps).all(), tau


def test_doubling_sigma_quadruples_the_added_covariance():
    c = chain_inputs()
    h = (c["span"][0, 1] - c["span"][0, 0]) / (c["K"] - 1)
    for tau in (np.inf, 5.0 * h):
        kw = dict(execution=EXEC, q=1e-7, m_var0=1e-4)
        P0_, _, _, _ = _chain(c, [0.0, tau], **kw)
        P1, _, Pb1, _ = _chain(c, [0.125, tau], **kw)
        P2, _, Pb2, _ = _chain(c, [0.25, tau], **kw)
        E, _, Eb = R.chain_error_bound(c["A"], c["Bn"], c["Bp"], c["G"], c["U"], c["units"], c["span"], C.P0_TEST, [0.25, tau], **kw)
        assert (np.abs((P2 - P0_) - 4.0 * (P1 - P0_)) <= 6.0 * E).all()          # (three chains, one of them four times)
        assert (np.abs(Pb2 - 4.0 * Pb1) <= 5.0 * Eb).all()
        Pt, _, _ = T.covariance_thrust_chain(c["A"], c["Bn"], c["Bp"], c["U"], c["units"], c["span"], C.P0_TEST, EXEC, q=1e-7, m_var0=1e-4)
        assert np.array_equal(P0_, Pt)                                               # sigma = 0: the thrust chain, to the bit


def test_statuses_and_fills_of_the_restatement():
    c = chain_inputs()
    rep = lambda a: np.repeat(a, 6, axis=0)
    dens = np.array([[0.1, np.inf], [-0.1, 10.0], [np.nan, 10.0], [0.1, 0.0], [0.1, np.nan], [np.inf, 5.0]])
    P, Pm, Pb, st = R.covariance_drag_chain(rep(c["A"]), rep(c["Bn"]), rep(c["Bp"]), rep(c["G"]), rep(c["U"]), rep(c["units"]), rep(c["span"]),
                                            C.P0_TEST, dens, ns=np.array([5, 30, 30, 30, 30, 30]))
    assert st.tolist() == [0] + [R.ST_NUMERIC] * 5
    assert np.isnan(P[1:]).all() and np.isnan(Pm[1:]).all() and np.isnan(Pb[1:]).all()
    assert (P[0, 5:] == 0.0).all() and (Pb[0, 5:] == 0.0).all() and np.isfinite(P[0]).all() and Pb[0, 4, 7] == 0.1 * 0.1


def test_python_surface_and_wrong_shapes():
    import mpconstellation_amd as pkg
    from mpconstellation_amd import _ffi, conjunction as cj
    assert "covariance_drag" in pkg.__all__ and callable(pkg.covariance_drag) and _ffi.NDENS == 2 and _ffi.FLAG_DRAG_COLUMN == 64
    assert {"mpcx_covariance_drag_workspace_bytes", "mpcx_covariance_drag_batch", "mpcx_covariance_drag_batch_dev"} <= set(_ffi.exported_symbols())
    S, K = 3, 5
    good = dict(Y=np.ones((S, 7, K)), units=np.ones((S, 2)), span=np.array([[0.0, 1.0]] * S), consts=np.ones((S, 8)), P0=np.eye(6), density=[0.1, np.inf])
    for bad, word in [(dict(density=np.zeros(3)), "density"), (dict(density=np.zeros((2, 2))), "density"), (dict(U=np.zeros((S, 3, 4))), "U"),
                      (dict(execution=np.zeros(4)), "execution"), (dict(mass_var0=[1.0, 2.0]), "mass_var0"), (dict(P0=np.eye(5)), "P0"),
                      (dict(q=-1.0), "q")]:
        with pytest.raises(ValueError, match=word):
            cj.covariance_drag(**{**good, **bad})
