"""Per-satellite problem options, host side (no GPU): the option table _ffi.make_popts builds for the *_sat entry points of
include/mpcx.h, ConstellationMPC's normalised_limits, and the way a multi-device call cuts the table."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_po_enum():
    """the MPCX_PO_* names of include/mpcx.h in their declared order (the last one is the count)"""
    txt = open(os.path.join(ROOT, "include", "mpcx.h")).read()
    body = re.search(r"enum\s*\{\s*(MPCX_PO_MIN_MASS.*?)\}", txt, flags=re.S).group(1)
    return [n.split("=")[0].strip() for n in body.split(",") if n.strip()]


def test_scalar_options_give_no_table():
    from mpconstellation_amd import _ffi
    assert _ffi.make_popts(None, 4) is None and _ffi.make_popts({}, 4) is None
    scalar = {"min_mass": 0.2, "u_lim": [0, 3.0], "r_lim": [0.95, 4.0], "eps_r": 1e-3, "eps_vr": 1e-6, "eps_vn": 1e-6,
              "eps_vt": 1e-6, "tf_max": 2.0, "w_nu": 10.0, "w_tr": 0.01, "r_des": 1.2}
    assert _ffi.make_popts(scalar, 4) is None
    assert _ffi.make_popts({"u_lim": np.array([0.0, 3.0]), "tf_max": np.float64(2.0)}, 4) is None
    assert _ffi.per_satellite_keys(scalar) == []


def test_column_order_is_the_headers():
    from mpconstellation_amd import _ffi
    names = header_po_enum()
    assert names[-1] == "MPCX_NPOPT" and len(names) == 12 and _ffi.NPOPT == 11
    for i, n in enumerate(names[:-1]):
        assert getattr(_ffi, n[len("MPCX_"):]) == i, n
        # ... and the order of mpcx_solve_opts' first eleven doubles
        assert _ffi.SolveOpts._fields_[i][0] == n[len("MPCX_PO_"):].lower() == _ffi.PO_FIELDS[i]
    # every column lands where its MPCX_PO_* index says, scalars and defaults broadcast
    S = 3
    opt = {"min_mass": [0.1, 0.2, 0.3], "u_lim": [[0, 1.0], [0, 2.0], [0, 3.0]], "r_lim": [[0.9, 4.0], [0.91, 4.1], [0.92, 4.2]],
           "eps_r": [1e-2, 1e-3, 1e-4], "eps_vr": [1e-5, 2e-5, 3e-5], "eps_vn": [4e-5, 5e-5, 6e-5], "eps_vt": [7e-5, 8e-5, 9e-5],
           "tf_max": [1.0, 2.0, 3.0], "w_nu": [10.0, 20.0, 30.0], "w_tr": [0.1, 0.2, 0.3]}
    t = _ffi.make_popts(opt, S)
    assert t.shape == (S, 11) and t.dtype == np.float64 and t.flags.c_contiguous
    assert t[:, _ffi.PO_MIN_MASS].tolist() == [0.1, 0.2, 0.3] and t[:, _ffi.PO_U_MAX].tolist() == [1.0, 2.0, 3.0]
    assert t[:, _ffi.PO_R_MIN].tolist() == [0.9, 0.91, 0.92] and t[:, _ffi.PO_R_MAX].tolist() == [4.0, 4.1, 4.2]
    assert t[:, _ffi.PO_EPS_R].tolist() == [1e-2, 1e-3, 1e-4] and t[:, _ffi.PO_EPS_VR].tolist() == [1e-5, 2e-5, 3e-5]
    assert t[:, _ffi.PO_EPS_VN].tolist() == [4e-5, 5e-5, 6e-5] and t[:, _ffi.PO_EPS_VT].tolist() == [7e-5, 8e-5, 9e-5]
    assert t[:, _ffi.PO_TF_MAX].tolist() == [1.0, 2.0, 3.0] and t[:, _ffi.PO_W_NU].tolist() == [10.0, 20.0, 30.0]
    assert t[:, _ffi.PO_W_TR].tolist() == [0.1, 0.2, 0.3]


def test_broadcasting_and_defaults():
    from mpconstellation_amd import _ffi, build
    S = 4
    t = _ffi.make_popts({"tf_max": np.array([1.0, 2.0, 3.0, 4.0]), "eps_r": 1e-6, "u_lim": [0, 0.3], "r_des": 1.5}, S)
    assert t.shape == (S, 11)
    assert t[:, _ffi.PO_TF_MAX].tolist() == [1.0, 2.0, 3.0, 4.0]
    assert (t[:, _ffi.PO_EPS_R] == 1e-6).all() and (t[:, _ffi.PO_U_MAX] == 0.3).all()
    # columns nobody named carry the library's defaults (mpcx_default_solve_opts)
    build.build()
    d = _ffi.make_solve_opts()
    for i, f in enumerate(_ffi.PO_FIELDS):
        if f not in ("tf_max", "eps_r", "u_max"):
            assert (t[:, i] == getattr(d, f)).all(), f
    # (S, 2) limits with scalar everything else; a (2,) limit beside an (S,) option
    t = _ffi.make_popts({"r_lim": np.array([[0.99, 5.0], [1.0, 4.0], [0.98, 3.0], [0.97, 2.0]])}, S)
    assert t[:, _ffi.PO_R_MIN].tolist() == [0.99, 1.0, 0.98, 0.97] and t[:, _ffi.PO_R_MAX].tolist() == [5.0, 4.0, 3.0, 2.0]
    assert (t[:, _ffi.PO_U_MAX] == d.u_max).all()
    t = _ffi.make_popts({"r_lim": [0.9, 3.0], "min_mass": [0.1, 0.2, 0.3, 0.4]}, S)
    assert (t[:, _ffi.PO_R_MIN] == 0.9).all() and (t[:, _ffi.PO_R_MAX] == 3.0).all()
    # the struct that goes with a table carries scalars (the first satellite's values); a uniform table's rows are that struct
    o = _ffi.make_solve_opts({"tf_max": np.array([1.5, 2.0, 3.0, 4.0]), "u_lim": np.array([[0, 0.3]] * 4), "w_tr": 0.004}, max_iter=50)
    assert (o.tf_max, o.u_max, o.w_tr, o.max_iter) == (1.5, 0.3, 0.004, 50)


def test_wrong_length_raises():
    from mpconstellation_amd import _ffi, ConstellationMPC, Satellite
    from mpconstellation_amd.optimizer import mpc_step_batch, solve_shared_tf
    for bad in ({"tf_max": [1.0, 2.0, 3.0]}, {"min_mass": np.ones((4, 1))}, {"u_lim": np.ones((3, 2))}, {"r_lim": np.ones((4, 3))},
                {"r_lim": np.ones((2, 4))}, {"eps_r": np.ones(5)}):
        with pytest.raises(ValueError):
            _ffi.make_popts(bad, 4)
    # where one final time serves all satellites, arrays are refused before anything reaches the library
    z = np.zeros
    with pytest.raises(ValueError):
        solve_shared_tf(z((2, 4, 7, 7)), z((2, 4, 7, 3)), z((2, 4, 7, 3)), z((2, 7, 4)), z((2, 7, 4)), z((2, 7, 5)), z((2, 3, 5)), [1.0, 1.0],
                        z((2, 8)), [1.0, 1.0], options={"tf_max": [1.0, 2.0]})
    with pytest.raises(ValueError):
        mpc_step_batch(z((2, 7, 5)), z((2, 3, 5)), [1.0, 1.0], z((2, 8)), [1.0, 1.0], options={"eps_r": [1e-3, 1e-4]}, shared_tf=True)
    sats = [Satellite(np.array([7e6, 0, 0]), np.array([0, 7.5e3, 0]), 100.0) for _ in range(3)]
    with pytest.raises(ValueError):
        ConstellationMPC(sats, options={"min_mass": [0.5, 0.5]})


def test_optimizer_with_several_satellites_refuses_arrays():
    from mpconstellation_amd import Optimizer

    class Scale:
        def get_normalized_constants(self): return None
    x = [np.zeros((7, 5)), np.zeros((7, 5))]
    opt = Optimizer(x, [np.zeros((3, 5))] * 2, None, 1.0, None, None, Scale(), verbose=False)
    with pytest.raises(ValueError):
        opt.solve_OPT({"tf_max": np.array([1.0, 2.0])})


def test_normalised_limits_hand_computed():
    """two satellites of different radius and mass under one physical keep-out radius, engine and dry mass"""
    from mpconstellation_amd import SatelliteScale, constants
    from mpconstellation_amd.constellation_mpc import normalised_limits
    states = [np.array([7.0e6, 0, 0, 0, 7.5e3, 0, 1000.0]), np.array([0, 0, 8.4e6, 6.9e3, 0, 0, 250.0])]
    scales = [SatelliteScale(x=s) for s in states]
    # the units by hand (satellite_scale.py:22-35): time = 2 pi sqrt(r^3 / mu), force = m r / time^2
    force = [m * r / (2 * np.pi * np.sqrt(r ** 3 / constants.MU_EARTH)) ** 2 for r, m in ((7.0e6, 1000.0), (8.4e6, 250.0))]
    o = normalised_limits(scales, r_min=6.678e6, u_max=2.0, min_mass=200.0)
    assert set(o) == {"r_lim", "u_lim", "min_mass"}
    assert o["r_lim"].shape == (2, 2) and o["u_lim"].shape == (2, 2) and o["min_mass"].shape == (2,)
    np.testing.assert_allclose(o["r_lim"][:, 0], [6.678e6 / 7.0e6, 6.678e6 / 8.4e6], rtol=1e-15)
    assert o["r_lim"][:, 1].tolist() == [5.0, 5.0]                                   # r_max not given: the default
    np.testing.assert_allclose(o["u_lim"][:, 1], [2.0 / force[0], 2.0 / force[1]], rtol=1e-14)
    assert o["u_lim"][:, 0].tolist() == [0.0, 0.0]
    np.testing.assert_allclose(o["min_mass"], [0.2, 0.8], rtol=1e-15)
    # per-satellite physical values, r_max alone; nothing given: nothing changed
    o = normalised_limits(scales, r_max=[2.1e7, 1.68e7])
    np.testing.assert_allclose(o["r_lim"], [[0.99, 3.0], [0.99, 2.0]], rtol=1e-15)
    assert set(o) == {"r_lim"} and normalised_limits(scales) == {}
    # ... and what it returns is a table the batched calls take
    from mpconstellation_amd import _ffi
    t = _ffi.make_popts(normalised_limits(scales, r_min=6.678e6, u_max=2.0), 2)
    np.testing.assert_allclose(t[:, _ffi.PO_U_MAX], [2.0 / force[0], 2.0 / force[1]], rtol=1e-14)
    assert t[0, _ffi.PO_MIN_MASS] == 0.1 and t[1, _ffi.PO_R_MAX] == 5.0


def test_table_is_cut_like_r_des():
    """devices=[...]: block `rank` of world = 3, S = 8 gets the rows of the table that belong to its r_des entries"""
    from mpconstellation_amd import _ffi
    from mpconstellation_amd.sharding import shard_block, sharded_call
    S, world = 8, 3
    r_des = 1.0 + 0.1 * np.arange(S)
    popts = _ffi.make_popts({"tf_max": 2.0 + np.arange(S), "u_lim": np.column_stack([np.zeros(S), 0.1 * (1 + np.arange(S))])}, S)
    seen = []
    fn = lambda r, po, device, slot, out: seen.append((r.copy(), po.copy(), slot))
    sharded_call(fn, [0] * world, [r_des, popts], {})
    assert len(seen) == world
    blocks = sorted(seen, key=lambda b: b[2])
    assert [len(b[0]) for b in blocks] == [3, 3, 2]
    for rank, (r, po, _) in enumerate(blocks):
        first, count = shard_block(S, world, rank)
        assert np.array_equal(r, r_des[first:first + count]) and np.array_equal(po, popts[first:first + count])
        assert po.shape == (count, 11)
        assert po[:, _ffi.PO_TF_MAX].tolist() == [2.0 + s for s in range(first, first + count)]
    assert np.array_equal(np.concatenate([b[1] for b in blocks]), popts)
    # scalar options: no table, and the blocks are told so
    seen.clear()
    sharded_call(lambda r, po, device, slot, out: seen.append(po), [0] * world, [r_des, _ffi.make_popts({"tf_max": 2.0}, S)], {})
    assert seen == [None, None, None]
