"""The oracle's drag branch and density model (oracle/dynamics.c: A_func's include_drag partials, ORACLE_FLAG_ATMO) against the
reference's own arrays, without a device: the fifteen cases of drag_discretize.npz, atmo_discretize.npz and atmo_propagate.npz,
and drag_edges.npz -- the reference on the inputs of tests/drag_cases.py (make_drag_edges_golden.py).  Then what makes those
inputs fit to hold a kernel to 1e-10 (tests/test_drag_oracle_gpu.py): each is sensitive, by >= 1e-7, to the term it is there
for, and none sits on a step-acceptance or floor knife edge -- a second build of the oracle with contracted multiply-adds takes
the same steps and agrees to 1e-11.  The figures are recorded in profiles/drag_oracle_checks.txt."""
import contextlib
import os
import platform
import subprocess

import numpy as np
import pytest

import drag_cases as D
import oracle_lib as O

RTOL = 1e-12                     # tests/test_oracle_golden.py
SENSITIVE = 1e-7                 # three orders above the device tolerance of 1e-10
HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = D.KEYS
relerr = D.relerr


def load(name):
    return np.load(os.path.join(HERE, "golden", name))


def check_nodes(o, counts, times, solver):
    """the accepted steps of the reference, node for node; times at test_oracle_golden.py's tolerance for the solver"""
    assert np.array_equal(o["node_counts"], np.ravel(counts))
    assert np.abs(o["node_t"] - times).max() < (1e-11 if solver == "RK23" else 1e-15)


def _flags(j2, solver):
    return O.FLAG_DRAG | (O.FLAG_J2 if j2 else 0) | (O.FLAG_RK23 if solver == "RK23" else 0)


@pytest.mark.parametrize("name", [str(c) for c in load("drag_discretize.npz")["cases"]])
def test_fixed_density_fixture(name):
    g = load("drag_discretize.npz")
    v = lambda k: g[f"{k}_{name}"]
    o = O.discretize(v("x"), v("u"), float(v("tf")), v("const"), _flags(bool(v("j2")), str(v("solver"))), uniform_steps=int(v("steps")), dump_nodes=True)
    assert o["status"] == 0
    for k in KEYS:
        assert o[k].shape == v(k).shape and relerr(o[k], v(k)) < RTOL, k
    if f"node_counts_{name}" in g:
        check_nodes(o, v("node_counts"), v("node_t"), str(v("solver")))
    # ... and drag reaches A now, not only Sigma
    plain = O.discretize(v("x"), v("u"), float(v("tf")), v("const"), _flags(bool(v("j2")), str(v("solver"))) & ~O.FLAG_DRAG, uniform_steps=int(v("steps")))
    assert abs(relerr(plain["A"], v("A")) / float(v("drag_share")) - 1) < 1e-6


@pytest.mark.parametrize("name", [str(c) for c in load("atmo_discretize.npz")["cases"]])
def test_atmosphere_fixture(name):
    g = load("atmo_discretize.npz")
    v = lambda k: g[f"{k}_{name}"]
    K = int(v("K"))
    x, u, atm = g[f"x_K{K}"], g[f"u_K{K}"], g[f"atmo_{str(v('model'))}"]
    flags = _flags(bool(v("j2")), str(v("solver")))
    o = O.discretize(x, u, float(v("tf")), v("const"), flags, uniform_steps=int(v("steps")), dump_nodes=True, atmosphere=atm)
    assert o["status"] == 0
    for k in KEYS:
        assert o[k].shape == v(k).shape and relerr(o[k], v(k)) < RTOL, k
    if f"node_counts_{name}" in g:
        check_nodes(o, v("node_counts"), v("node_t"), str(v("solver")))
    if f"position_share_{name}" in g:
        # the shares the generator measured with the reference, from the oracle
        for key, other in (("drag_share", dict(flags=flags & ~O.FLAG_DRAG)), ("position_share", dict(flags=flags | O.FLAG_NO_DRHO, atmosphere=atm)),
                           ("fixed_density_share", dict(flags=flags))):
            a = O.discretize(x, u, float(v("tf")), v("const"), uniform_steps=int(v("steps")), **other)["A"]
            assert abs(relerr(a, o["A"]) / float(v(key)) - 1) < 1e-6, key


@pytest.mark.parametrize("name", [str(c) for c in load("atmo_propagate.npz")["cases"]])
def test_atmosphere_rollout_fixture(name):
    p = load("atmo_propagate.npz")
    ctrl = O.make_ctrl(O.CTRL_TANGENTIAL, (0.5, 0, 0)) if str(p[f"law_{name}"]) == "tan" else O.make_ctrl(O.CTRL_SEQUENCE, useq=p["useq"], end_tau=1.0)
    y, rc, _ = O.propagate(p["y0"], 1.0, p["const"], ctrl, int(p["n_eval"]), O.FLAG_DRAG | O.FLAG_J2, atmosphere=p[f"atmo_{str(p[f'model_{name}'])}"])
    assert rc == 0 and np.abs(y - p[f"y_{name}"]).max() < 1e-12          # (test_oracle_golden.py::test_propagate)


def test_atmosphere_argument():
    """atmosphere= takes an Atmosphere or its four numbers; None and the old entry points are the fixed density"""
    b = D.batch()
    x, u, cst = b["x"][0][:, 3], b["u"][0][:, 3], b["const"][0]
    atm = D.models()["general"]
    A = O.A_func(x, u, 0.7, cst, O.FLAG_DRAG, atmosphere=atm)
    assert np.array_equal(A, O.A_func(x, u, 0.7, cst, O.FLAG_DRAG, atmosphere=atm.coefficients()))
    fixed = np.zeros((7, 7))
    O.lib().oracle_A_func(O._p(O._c(x)), O._p(O._c(u)), 0.7, O._p(O._c(cst)), O.FLAG_DRAG, O._p(fixed))
    assert np.array_equal(fixed, O.A_func(x, u, 0.7, cst, O.FLAG_DRAG)) and relerr(A, fixed) > 1e-3
    assert np.array_equal(fixed, O.A_func(x, u, 0.7, cst, O.FLAG_DRAG | O.FLAG_ATMO))       # the bit without a model
    with pytest.raises(ValueError):
        O.A_func(x, u, 0.7, cst, O.FLAG_DRAG, atmosphere=(1.0, 2.0, 3.0))


@pytest.mark.parametrize("model", ["fixed", "power", "general", "floor"])
def test_drag_jacobian_is_the_derivative_of_the_dynamics(model):
    """A_func with drag against central differences of oracle_dynamics, tf != 1, u not parallel to v: on a point above the floor,
    and (floor) on one below it, where the position block is zero"""
    b = D.batch()
    atm = D.floor_model() if model == "floor" else D.models()[model]
    x, u, cst, tf = b["x"][4][:, 5].copy(), b["u"][4][:, 5], b["const"][4], 1.25
    assert (D.altitude(x, cst) < D.H_FLOOR) and D.altitude(x, cst) > 1e5 + 1e3
    A = O.A_func(x, u, tf, cst, O.FLAG_DRAG | O.FLAG_J2, atmosphere=atm)
    J = np.zeros((7, 7))
    for j in range(7):
        h = 1e-6 * max(abs(x[j]), 1.0)
        e = np.zeros(7); e[j] = h
        J[:, j] = (O.dynamics(x + e, u, tf, cst, O.FLAG_DRAG | O.FLAG_J2, atmosphere=atm)[0] - O.dynamics(x - e, u, tf, cst, O.FLAG_DRAG | O.FLAG_J2, atmosphere=atm)[0]) / (2 * h)
    drag = A - O.A_func(x, u, tf, cst, O.FLAG_J2)
    assert np.abs(A - J).max() < 1e-6 * np.abs(drag).max(), np.abs(A - J).max() / np.abs(drag).max()
    xi = O.xi_func(x, u, tf, cst, O.FLAG_DRAG | O.FLAG_J2, atmosphere=atm)
    assert np.abs(xi + A @ x + O.B_func(x, u, tf, cst) @ u).max() < 1e-12 * np.abs(xi).max()
    assert (np.abs(drag[3:6, 0:3]).max() == 0.0) == (model in ("fixed", "floor"))


# ---- drag_edges.npz: the reference on the inputs the device tests use ------------------------------------------------------------

def test_edges_inputs_are_the_shared_inputs():
    """the fixture's inputs are those of drag_cases.py (which rebuilds them with the oracle's rollout: rounding apart at most)"""
    g = load("drag_edges.npz")
    same = lambda a, b: np.allclose(a, b, rtol=1e-11, atol=1e-13)
    b = D.batch()
    assert all(same(g[f"batch_{k}"], b[k]) for k in ("x", "u", "tf", "const", "y0"))
    for tf in D.FLOOR_TFS:
        c = D.floor_case(tf)
        assert all(same(g[f"floor_{k}_tf{int(tf)}"], c[k]) for k in ("x", "u", "const", "y0"))
    c = D.rollout_case()
    assert all(same(g[f"roll_{k}"], c[k]) for k in ("y0", "const", "tf", "n_eval", "end_tau", "constant", "tangential", "sequence"))
    assert same(g["roll_atmo"], D.models()["general"].coefficients()) and same(g["floor_atmo"], D.floor_model().coefficients())
    assert [str(t) for t in g["batch_configs"]] == ["/".join([m, s, "j2" if j else "nj2"]) for m, s, j in D.REFERENCE_CONFIGS]


@pytest.mark.parametrize("config", D.REFERENCE_CONFIGS, ids=lambda c: "-".join(map(str, c)))
def test_edges_batch(config):
    """random thrust directions, tf in [0.5, 1.5], other R0 / RHO, the all-zero thrust table; the general model"""
    g = load("drag_edges.npz")
    model, solver, j2 = config
    tag = "/".join([model, solver, "j2" if j2 else "nj2"])
    atm = None if model == "fixed" else g[f"batch_atmo_{model}"]
    at = 0
    for s in range(g["batch_x"].shape[0]):
        o = D.oracle_discretize(g["batch_x"][s], g["batch_u"][s], g["batch_tf"][s], g["batch_const"][s], atm, solver, j2, dump_nodes=True)
        assert o["status"] == 0
        for k in KEYS:
            assert relerr(o[k], g[f"batch_{k}_{tag}"][s]) < RTOL, (s, k)
        if solver != "uni11":
            n = int(o["node_counts"].sum())
            check_nodes(o, g[f"batch_node_counts_{tag}"][s], g[f"batch_node_t_{tag}"][at:at + n], "RK23" if solver == "rk23" else "RK45")
            at += n


@pytest.mark.parametrize("solver", ["rk45", "rk23"])
@pytest.mark.parametrize("tf", D.FLOOR_TFS)
def test_edges_floor_crossing(tf, solver):
    g = load("drag_edges.npz")
    t = f"tf{int(tf)}"
    o = D.oracle_discretize(g[f"floor_x_{t}"], g[f"floor_u_{t}"], tf, g[f"floor_const_{t}"], g["floor_atmo"], solver, True, dump_nodes=True)
    assert o["status"] == 0
    for k in KEYS:
        assert relerr(o[k], g[f"floor_{k}_{t}_{solver}"]) < RTOL, k
    check_nodes(o, g[f"floor_node_counts_{t}_{solver}"], g[f"floor_node_t_{t}_{solver}"], "RK23" if solver == "rk23" else "RK45")
    assert set(D.interval_kinds(o, g[f"floor_const_{t}"], D.FLOOR_K)) == {"on", "cross", "above"}
    if solver == "rk45":
        y, rc, _ = O.propagate(g[f"floor_y0_{t}"], tf, g[f"floor_const_{t}"], O.make_ctrl(O.CTRL_SEQUENCE, useq=g[f"floor_u_{t}"], end_tau=1.0), 20,
                               O.FLAG_DRAG | O.FLAG_J2, atmosphere=g["floor_atmo"])
        assert rc == 0 and np.abs(y - g[f"floor_y_{t}"]).max() < 1e-12


@pytest.mark.parametrize("j2", [False, True])
@pytest.mark.parametrize("law", D.LAWS)
def test_edges_rollouts(law, j2):
    """every thrust law through the general model, tf = 0.5, 1, 2, drag without and with J2"""
    g = load("drag_edges.npz")
    c = {k: g[f"roll_{k}"] for k in ("y0", "const", "tf", "n_eval", "end_tau", "constant", "tangential", "sequence")}
    for s in range(3):
        y, _ = D.oracle_rollout(law, c, s, j2, model=g["roll_atmo"])
        assert np.abs(y - g[f"roll_y_{law}_{'j2' if j2 else 'nj2'}_{s}"]).max() < 1e-12, s


# ---- what makes the inputs fit for a 1e-10 comparison --------------------------------------------------------------------------

def disc_inputs():
    """every discretize input of tests/test_drag_oracle_gpu.py: (name, x, u, tf, const, model, solver, j2, claims) -- claims: the
    satellite is there to test the drag terms (S x 1e4)"""
    b = D.batch()
    for model, solver, j2 in D.BATCH_CONFIGS:
        for s in range(5):
            yield f"batch {model}/{solver}/{'j2' if j2 else 'nj2'} sat {s}", b["x"][s], b["u"][s], b["tf"][s], b["const"][s], model, solver, j2, bool(D.BIG_S[s])
    for tf in D.FLOOR_TFS:
        c = D.floor_case(tf)
        for solver in ("rk45", "rk23"):
            yield f"floor tf {tf} {solver}", c["x"], c["u"], tf, c["const"], D.floor_model(), solver, True, True
    for s, K in D.SMALL:
        c = D.short_case(s, K)
        yield f"short K {K}", c["x"], c["u"], c["tf"], c["const"], "general", "rk45", True, True
    for s, K in zip(D.STAGE_SATS, D.STAGE_KS):
        c = D.short_case(s, int(K))
        for model, j2 in (("fixed", False), ("fixed", True), ("general", False), ("general", True)):
            yield f"stage K {K} {model} {'j2' if j2 else 'nj2'}", c["x"], c["u"], c["tf"], c["const"], model, "rk45", j2, True
    for model in ("fixed", "general"):
        c = D.step_case(model)
        for s in range(3):
            yield f"step {model} sat {s}", c["x"][s], c["u"][s], c["tf"][s], c["const"][s], model, "rk45", False, True


def shares(x, u, tf, cst, model, solver, j2):
    """relative change of A with the drag off, with drho = 0, with the fixed density (the last two: 0 under the fixed density)"""
    atm = D.models()[model] if isinstance(model, str) else model
    flags, steps = D.oracle_flags(model, solver, j2), D.SOLVERS[solver][1]
    A = O.discretize(x, u, tf, cst, flags, uniform_steps=steps, atmosphere=atm)["A"]
    off = relerr(O.discretize(x, u, tf, cst, flags & ~O.FLAG_DRAG, uniform_steps=steps)["A"], A)
    if atm is None:
        return off, 0.0, 0.0
    return (off, relerr(O.discretize(x, u, tf, cst, flags | O.FLAG_NO_DRHO, uniform_steps=steps, atmosphere=atm)["A"], A),
            relerr(O.discretize(x, u, tf, cst, flags, uniform_steps=steps)["A"], A))


def test_every_input_is_sensitive_to_its_terms(capsys):
    lines = []
    for name, x, u, tf, cst, model, solver, j2, claims in disc_inputs():
        off, pos, fixed = shares(x, u, float(tf), cst, model, solver, j2)
        lines.append(f"{name}: drag {off:.2e} position block {pos:.2e} fixed density {fixed:.2e}" + ("" if claims else "  (claims nothing)"))
        if claims:
            assert off >= SENSITIVE and (model == "fixed" or (pos >= SENSITIVE and fixed >= SENSITIVE)), lines[-1]
    # the floor: against the same model with its floor below the orbit
    for tf in D.FLOOR_TFS:
        c, m = D.floor_case(tf), D.floor_model()
        low = (m.c0, m.c1, m.c2, 1e5)
        for solver in ("rk45", "rk23"):
            d = relerr(D.oracle_discretize(c["x"], c["u"], tf, c["const"], low, solver, True)["A"], D.oracle_discretize(c["x"], c["u"], tf, c["const"], m, solver, True)["A"])
            lines.append(f"floor tf {tf} {solver}: against the model without the floor {d:.2e}")
            assert d >= SENSITIVE
        y = O.propagate(c["y0"], tf, c["const"], O.make_ctrl(O.CTRL_SEQUENCE, useq=c["u"], end_tau=1.0), 20, O.FLAG_DRAG | O.FLAG_J2, atmosphere=m)[0]
        y0 = O.propagate(c["y0"], tf, c["const"], O.make_ctrl(O.CTRL_SEQUENCE, useq=c["u"], end_tau=1.0), 20, O.FLAG_DRAG | O.FLAG_J2, atmosphere=low)[0]
        lines.append(f"floor tf {tf} rollout: end state against the model without the floor {np.abs(y - y0)[:, -1].max():.2e}")
        assert np.abs(y - y0)[:, -1].max() >= SENSITIVE
    # rollouts: the end state against the fixed density and against no drag
    c = D.rollout_case()
    for law in D.LAWS:
        for j2 in (False, True):
            for s in range(3):
                y = D.oracle_rollout(law, c, s, j2)[0][:, -1]
                fixed = np.abs(y - D.oracle_rollout(law, c, s, j2, model="fixed")[0][:, -1]).max()
                off = np.abs(y - O.propagate(c["y0"][s], float(c["tf"][s]), c["const"][s], D.oracle_ctrl(law, c, s), int(c["n_eval"][s]), O.FLAG_J2 if j2 else 0)[0][:, -1]).max()
                lines.append(f"rollout {law} {'j2' if j2 else 'nj2'} sat {s}: end state against the fixed density {fixed:.2e}, against no drag {off:.2e}")
                assert fixed >= SENSITIVE and off >= SENSITIVE, lines[-1]
    with capsys.disabled():
        print("\n" + "\n".join(lines))


@contextlib.contextmanager
def contracted_build(tmp_path):
    """the oracle's sources compiled a second time with -ffp-contract=fast (and the machine's fused multiply-add), into tmp_path,
    as the library oracle_lib calls inside the block"""
    flags = ["-O2", "-fPIC", "-std=gnu11", "-ffp-contract=fast", "-fno-fast-math"]
    if platform.machine() in ("x86_64", "AMD64"):
        with open("/proc/cpuinfo") as f:
            if " fma " in f.read().replace("\n", " "):
                flags.append("-mfma")
    so = str(tmp_path / "liboracle_contracted.so")
    srcs = sorted(os.path.join(O.ORACLE_DIR, f) for f in os.listdir(O.ORACLE_DIR) if f.endswith(".c"))
    subprocess.check_call([os.environ.get("CC", "cc"), *flags, "-shared", "-o", so, *srcs, "-lm"])
    O.lib()
    keep, env = O._lib, os.environ.get("ORACLE_LIB")
    O._lib, os.environ["ORACLE_LIB"] = None, so
    try:
        O.lib()
        yield
    finally:
        O._lib = keep
        if env is None:
            del os.environ["ORACLE_LIB"]
        else:
            os.environ["ORACLE_LIB"] = env


def test_no_input_sits_on_a_knife_edge(tmp_path, capsys):
    """both builds of the oracle take the same steps on every input and agree to 1e-11: a device whose rounding differs from the
    oracle's by as much as a contracted multiply-add does will accept the same steps and land on the same side of the floor"""
    def everything():
        out = {}
        for name, x, u, tf, cst, model, solver, j2, _ in disc_inputs():
            o = D.oracle_discretize(x, u, float(tf), cst, model, solver, j2)
            out[name] = (o["node_counts"].copy(), o["node_nfev"].copy(), [o[k] for k in KEYS])
        c = D.rollout_case()
        for law in D.LAWS:
            for j2 in (False, True):
                for s in range(3):
                    y, ns = D.oracle_rollout(law, c, s, j2)
                    out[f"rollout {law} {'j2' if j2 else 'nj2'} sat {s}"] = (np.array([ns]), np.array([0]), [y])
        for tf in D.FLOOR_TFS:
            c = D.floor_case(tf)
            y, rc, ns = O.propagate(c["y0"], tf, c["const"], O.make_ctrl(O.CTRL_SEQUENCE, useq=c["u"], end_tau=1.0), 20, O.FLAG_DRAG | O.FLAG_J2, atmosphere=D.floor_model())
            out[f"floor tf {tf} rollout"] = (np.array([ns]), np.array([0]), [y])
        return out
    a = everything()
    with contracted_build(tmp_path):
        b = everything()
    worst, differ = ("", 0.0), 0
    for name in a:
        assert np.array_equal(a[name][0], b[name][0]) and np.array_equal(a[name][1], b[name][1]), name
        for p, q in zip(a[name][2], b[name][2]):
            differ += not np.array_equal(p, q)
            e = np.abs(p - q).max() if name.startswith("rollout") or name.endswith("rollout") else relerr(q, p)
            worst = max(worst, (name, e), key=lambda t: t[1])
            assert e < 1e-11, (name, e)
    with capsys.disabled():
        print(f"\ntwo builds: {len(a)} inputs, same step counts on all; {differ} arrays differ in some bit; worst disagreement {worst[1]:.2e} ({worst[0]})")
