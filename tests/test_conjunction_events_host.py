"""screen_events in front of the library -- the argument checks it shares with screen_pairs and its own, the empty list -- and the
host-side pieces around it, cumulative_probability and EncounterEvents' compaction of the library's padded blocks.  No device."""
import numpy as np
import pytest


def sides():
    eph, cat = np.zeros((3, 6, 5)), np.zeros((4, 6, 5))
    traj = dict(Y=np.zeros((3, 7, 8)), units=np.ones((3, 2)), span=np.tile([0.0, 1.0], (3, 1)))
    return eph, cat, traj


def test_an_empty_list_needs_no_device():
    from mpconstellation_amd import screen_events, ConjunctionResult, EncounterEvents
    eph, cat, traj = sides()
    ev = screen_events(np.zeros((0, 4)), 0.0, 1.0, threshold=5e3, eph=eph, cat_eph=cat)
    assert isinstance(ev, EncounterEvents) and ev.events.shape == (0, 4) and ev.events.dtype == np.float64
    assert ev.row.shape == ev.interval.shape == ev.edge.shape == (0,) and ev.edge.dtype == bool
    assert ev.count.shape == ev.truncated.shape == ev.status.shape == (0,) and ev.status.dtype == np.int32 and ev.max_events == 16
    empty = ConjunctionResult(np.zeros(3), np.zeros(3, dtype=np.int32), np.zeros(3), np.zeros((0, 4)), 0)
    ev = screen_events(empty, 0.0, 1.0, max_events=3, M=5, **traj)
    assert ev.events.shape == (0, 4) and ev.eph_status is None and ev.cat_status is None and ev.max_events == 3


def test_arguments_are_checked_before_the_library_is_called():
    from mpconstellation_amd import screen_events
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
                    (one, dict(M=5, Y=traj["Y"], units=np.ones((2, 2)), span=traj["span"])),
                    (one, dict(eph=eph, max_events=0)),
                    (one, dict(eph=eph, max_events=-2)),
                    (one, dict(eph=eph, max_events=2.5)),
                    (one, dict(eph=eph, threshold=np.nan)),
                    (np.zeros((0, 4)), dict(eph=eph, max_events=0)),         # (an empty list is checked like any other)
                    (np.zeros((0, 4)), dict(eph=eph, threshold=np.nan))):
        with pytest.raises(ValueError):
            screen_events(bad, 0.0, 1.0, **kw)
    with pytest.raises(ValueError, match="screen_events"):
        screen_events(one, 0.0, 1.0)
    with pytest.raises(ValueError):
        screen_events(one, 1.0, 1.0, eph=eph)
    with pytest.raises(ValueError):
        screen_events(one, None, 1.0, eph=eph)


def padded():
    """three list rows with E = 3 slots: two events, none (a bad row), five found of which three are stored"""
    nan = np.nan
    events = np.array([[[0, 1, 10.0, 1.0], [0, 1, 30.0, 7.0], [0, 1, nan, nan]],
                       [[2, 2, nan, nan], [2, 2, nan, nan], [2, 2, nan, nan]],
                       [[4, 3, 5.0, 0.0], [4, 3, 6.0, 2.5], [4, 3, 7.0, 9.0]]])
    info = np.array([[[3, 0], [40, 0], [-1, 0]], [[-1, 0]] * 3, [[0, 1], [17, 0], [64, 0]]], dtype=np.int32)
    return events, info, np.array([2, 0, 5], dtype=np.int32), np.array([0, 9, 0], dtype=np.int32)


def test_encounter_events_compacts_the_padded_blocks():
    from mpconstellation_amd import EncounterEvents
    events, info, count, status = padded()
    ev = EncounterEvents(events, info, count, status)
    assert ev.events.tolist() == [[0, 1, 10.0, 1.0], [0, 1, 30.0, 7.0], [4, 3, 5.0, 0.0], [4, 3, 6.0, 2.5], [4, 3, 7.0, 9.0]]
    assert ev.events.flags.c_contiguous and ev.events.dtype == np.float64
    assert ev.row.tolist() == [0, 0, 2, 2, 2] and ev.interval.tolist() == [3, 40, 0, 17, 64]
    assert ev.edge.tolist() == [False, False, True, False, False] and ev.edge.dtype == bool
    assert ev.count.tolist() == [2, 0, 5] and ev.truncated.tolist() == [False, False, True] and ev.status.tolist() == [0, 9, 0]
    assert ev.max_events == 3 and ev.eph_status is None and ev.cat_status is None and "5 of 7" in repr(ev)
    with pytest.raises(ValueError):
        EncounterEvents(events, info[:, :2], count, status)


def test_cumulative_probability():
    from mpconstellation_amd import EncounterEvents, cumulative_probability
    from mpconstellation_amd.conjunction import CollisionResult
    ev = EncounterEvents(*padded())
    pc = np.array([0.5, 0.5, 1e-9, 2e-9, 3e-9])
    cum = cumulative_probability(ev, pc)
    assert cum.shape == (3,) and abs(cum[0] - 0.75) <= 4 * np.finfo(np.float64).eps and cum[1] == 0.0 and not np.signbit(cum[1])
    exact = 6e-9 - 11e-18 + 6e-27                                    # 1 - (1 - a)(1 - b)(1 - c) expanded: no cancellation
    assert abs(cum[2] - exact) <= 4 * np.finfo(np.float64).eps * exact
    cum = cumulative_probability(ev, np.array([0.5, np.nan, 0.0, 0.0, 0.0]))
    assert np.isnan(cum[0]) and cum[1] == 0.0 and cum[2] == 0.0
    assert cumulative_probability(ev, np.array([1.0, 0.25, 0.0, 1.0, 0.5])).tolist() == [1.0, 0.0, 1.0]
    out = np.zeros((5, 6)); out[:, 0] = pc
    assert cumulative_probability(ev, CollisionResult(ev.events, out, np.zeros(5, dtype=np.int32))).tobytes() == cumulative_probability(ev, pc).tobytes()
    with pytest.raises(ValueError):
        cumulative_probability(ev, pc[:4])


def test_the_binding_and_the_exports_name_the_new_entry_points():
    import mpconstellation_amd as pkg
    from mpconstellation_amd import _ffi
    names = {"mpcx_conjunction_events" + tail for tail in ("", "_dev", "_traj", "_traj_dev", "_workspace_bytes")}
    assert names <= set(_ffi.exported_symbols())
    assert {"screen_events", "EncounterEvents", "cumulative_probability"} <= set(pkg.__all__)
    assert callable(pkg.ConstellationMPC.encounters)
