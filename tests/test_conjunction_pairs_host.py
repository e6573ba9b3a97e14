"""screen_pairs in front of the library: the argument checks and the empty list, which need no device."""
import numpy as np
import pytest


def sides():
    eph, cat = np.zeros((3, 6, 5)), np.zeros((4, 6, 5))
    traj = dict(Y=np.zeros((3, 7, 8)), units=np.ones((3, 2)), span=np.tile([0.0, 1.0], (3, 1)))
    return eph, cat, traj


def test_an_empty_list_needs_no_device():
    from mpconstellation_amd import screen_pairs, ConjunctionResult
    eph, cat, traj = sides()
    out, status = screen_pairs(np.zeros((0, 4)), 0.0, 1.0, eph=eph, cat_eph=cat)
    assert out.shape == (0, 4) and out.dtype == np.float64 and status.shape == (0,) and status.dtype == np.int32
    empty = ConjunctionResult(np.zeros(3), np.zeros(3, dtype=np.int32), np.zeros(3), np.zeros((0, 4)), 0)
    out, status, eph_status, cat_status = screen_pairs(empty, 0.0, 1.0, M=5, **traj)
    assert out.shape == (0, 4) and status.shape == (0,) and eph_status is None and cat_status is None


def test_arguments_are_checked_before_the_library_is_called():
    from mpconstellation_amd import screen_pairs
    eph, cat, traj = sides()
    one = np.zeros((1, 4))
    for bad, kw in ((np.zeros((2, 3)), dict(eph=eph)),               # a list that is not (n, 4)
                    (one, dict()),                                   # neither form
                    (one, dict(eph=eph, M=5, **traj)),               # both forms
                    (one, dict(cat_eph=cat)),                        # a catalogue alone
                    (one, dict(eph=eph, cat_eph=np.zeros((4, 6, 6)))),       # two grids
                    (one, dict(eph=eph, M=4)),                       # M beside an ephemeris that has another
                    (one, dict(eph=np.zeros((3, 5, 5)))),
                    (one, dict(**traj)),                             # trajectories without M
                    (one, dict(M=1, **traj)),
                    (one, dict(M=5, cat_Y=np.zeros((4, 7, 8)), **traj)),     # a catalogue without units and span
                    (one, dict(M=5, Y=traj["Y"], units=np.ones((2, 2)), span=traj["span"]))):
        with pytest.raises(ValueError):
            screen_pairs(bad, 0.0, 1.0, **kw)
    with pytest.raises(ValueError):
        screen_pairs(one, 1.0, 1.0, eph=eph)
    with pytest.raises(ValueError):
        screen_pairs(one, None, 1.0, eph=eph)
