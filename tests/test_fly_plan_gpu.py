"""ConstellationMPC.fly_plan: the stored plan flown under the truth model with run_segment's bookkeeping and without its update.
Everything is compared bit for bit: update + fly_plan is what run_segment does (its separate-flight path plays the same table
through the same propagate kernel with the same arguments, and test_mpc_loop_gpu.py holds that path to the fused one byte for
byte), so no tolerance appears here."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KW = dict(base_res=30, tf_horizon=2, tf_interval=1, r_des=1.5, sim_base_res=50)


def make():
    from mpconstellation_amd import Satellite
    from mpconstellation_amd.constellation import constellation_states
    st = constellation_states(4096)[[3, 500, 1234]]
    return [Satellite(s[:3].copy(), s[3:6].copy(), float(s[6])) for s in st]


def by_hand(mpc, y0, U, tf=1, n_eval=50):
    from mpconstellation_amd import propagate_batch, _ffi
    y, status, _ = propagate_batch(y0, tf, mpc.consts, (_ffi.CTRL_SEQUENCE, U, U.shape[2], mpc.plan_tf / mpc.interval), n_eval,
                                   mpc.include_drag, mpc.include_J2, 0.001, mpc.device, Kus=mpc.plan_K)
    assert (status == 0).all()
    return y


def same_flight(a, b):
    assert len(a._seg_y) == len(b._seg_y)
    for ya, yb, ta, tb in zip(a._seg_y, b._seg_y, a._seg_t, b._seg_t):
        assert ya.tobytes() == yb.tobytes() and ta.tobytes() == tb.tobytes()
    assert a._seg_tf == b._seg_tf
    for sa, sb in zip(a.sats, b.sats):
        assert np.array_equal(sa.get_state_vector(), sb.get_state_vector())
        assert np.array_equal(a.sim_data[sa.id], b.sim_data[sb.id]) and np.array_equal(a.sim_time[sa.id], b.sim_time[sb.id])


def test_update_then_fly_plan_is_run_segment():
    from mpconstellation_amd import ConstellationMPC
    a, b = ConstellationMPC(make(), **KW), ConstellationMPC(make(), **KW)
    a.run_segment(1)
    y0 = b._y0()
    assert b.update() is None and b.horizon == 1                     # (the update shrank the horizon; fly_plan leaves it alone)
    want = by_hand(b, y0, b._plan[1])
    b.fly_plan(1)
    assert b.horizon == 1 and b._seg_y[-1].tobytes() == want.tobytes() and b._seg_y[-1].shape == (3, 7, 50)
    same_flight(a, b)
    assert np.array_equal(a.plan_tf, b.plan_tf) and all(np.array_equal(x, y) for x, y in zip(a.plan_u, b.plan_u))
    a.run_segment(1); b.run_segment(1)                               # a second segment: the bookkeeping left the same state behind
    same_flight(a, b)
    assert a.sim_data[a.sats[0].id].shape == (7, 100)


def test_fly_plan_flies_the_table_the_instance_holds():
    """a plan put in the instance's place (what adopting a changed thrust table does) is what fly_plan flies; a second fly_plan
    plays the table again from the new state and continues the clock as run_segment does"""
    from mpconstellation_amd import ConstellationMPC
    mpc = ConstellationMPC(make(), **KW)
    with pytest.raises(ValueError):
        mpc.fly_plan(1)
    mpc.update()
    X, U, NU = mpc._plan
    changed = 0.5 * U
    mpc._plan = (X, changed, NU); mpc._plan_lists = None
    y0 = mpc._y0()
    want = by_hand(mpc, y0, changed)
    assert want.tobytes() != by_hand(mpc, y0, U).tobytes()
    mpc.fly_plan(1)
    assert mpc._seg_y[0].tobytes() == want.tobytes() and all(np.array_equal(u, changed[s][:, :mpc.plan_K[s]]) for s, u in enumerate(mpc.plan_u))
    f = mpc._f
    end = np.column_stack([want[:, 0:3, -1] * f[:, 0:1], want[:, 3:6, -1] * f[:, 1:2], want[:, 6, -1] * f[:, 2]])
    assert all(np.array_equal(sat.get_state_vector(), end[i]) for i, sat in enumerate(mpc.sats))
    y1 = mpc._y0()
    mpc.fly_plan(0.5)
    assert mpc._seg_y[1].tobytes() == by_hand(mpc, y1, changed, tf=0.5, n_eval=25).tobytes() and mpc._seg_tf == [1.0, 0.5]
    assert np.array_equal(mpc._seg_t[1], np.linspace(0, 1, 25) + mpc._seg_t[0][-1] * 0.5 + 0.0000001)
    assert mpc.sim_data[mpc.sats[0].id].shape == (7, 75) and mpc.horizon == 1
