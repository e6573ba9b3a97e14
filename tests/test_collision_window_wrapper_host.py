"""collision_probability_window's wrappers without a device: every bad argument is a ValueError before the library (which needs a
device) is touched, an empty list never reaches it, encounter_half_window, and cumulative_probability on the new result."""
import numpy as np
import pytest

from mpconstellation_amd import conjunction as cj, _ffi

S, N = 2, 5
Y, UNITS, SPAN, P = np.zeros((S, 7, N)), np.ones((S, 2)), np.array([[0.0, 1.0]] * S), np.zeros((S, N, 6, 6))
GOOD = dict(pairs=np.array([[0.0, 1.0, 100.0, 0.5]]), radius=5.0, Y=Y, units=UNITS, span=SPAN, P=P, half_window=10.0)


def test_argument_checks():
    bad = [dict(pairs=np.zeros((1, 3))), dict(pairs=np.zeros(4)), dict(radius=[1.0, 2.0, 3.0]), dict(P=np.zeros((S, N, 6, 5))),
           dict(P=np.zeros((S, N + 1, 6, 6))), dict(Y=np.zeros((S, 7, 1)), P=np.zeros((S, 1, 6, 6))), dict(mu=0.0), dict(ns=[5]),
           dict(cat=(Y, UNITS, SPAN, P)), dict(cat=(Y, UNITS, SPAN, np.zeros((S, N, 6)), 1.0)), dict(cat=(Y, UNITS, np.ones((S, 3)), P, 1.0)),
           dict(cat=(Y, UNITS, SPAN, P, [1.0, 2.0, 3.0])),
           dict(half_window=None), dict(half_window=[1.0, 2.0]), dict(half_window=np.ones((1, 1))),
           dict(panels=0), dict(panels=-1), dict(panels=1.5), dict(panels=_ffi.PW_MAX_PANELS + 1), dict(panels=[4])]
    for kw in bad:
        with pytest.raises(ValueError):
            cj.collision_probability_window(**{**GOOD, **kw})
    with pytest.raises(ValueError, match=r"half_window.*\(1,\)"):
        cj.collision_probability_window(**{**GOOD, "half_window": [1.0, 2.0]})
    with pytest.raises(ValueError, match="panels.*1 .. 64"):
        cj.collision_probability_window(**{**GOOD, "panels": 65})


def test_the_empty_list_makes_no_library_call(monkeypatch):
    def no_call(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_ffi, "call", no_call)
    monkeypatch.setattr(_ffi, "context", no_call)
    empty_scr = cj.ConjunctionResult(np.zeros(S), np.zeros(S, dtype=np.int32), np.zeros(S), cj.sort_pairs([]), 0)
    empty_ev = cj.EncounterEvents(np.zeros((3, 2, 4)), np.zeros((3, 2, 2), dtype=np.int32), np.zeros(3, dtype=np.int32), np.zeros(3, dtype=np.int32))
    for kw in (dict(), dict(cat=(Y, UNITS, SPAN, P, 1.0)), dict(devices=[0, 0]), dict(pairs=empty_scr), dict(pairs=empty_ev), dict(half_window=np.zeros(0))):
        r = cj.collision_probability_window(**{**GOOD, "pairs": np.zeros((0, 4)), **kw})
        assert isinstance(r, cj.WindowCollisionResult)
        assert r.p.shape == r.start.shape == r.entries.shape == r.rate_max.shape == r.t_rate_max.shape == r.status.shape == (0,)
        assert r.window.shape == (0, 2) and r.pairs.shape == (0, 4) and r.status.dtype == np.int32
    with pytest.raises(AssertionError, match="the library was called"):   # (a list with a row does reach it)
        cj.collision_probability_window(**GOOD)


def test_result_columns_and_event_rows(monkeypatch):
    """the wrapper hands the library one row per stored event of an EncounterEvents and maps the columns by name"""
    seen = {}

    def fake_call(name, ctx, n, *args):
        seen.update(name=name, n=n, panels=args[-3])
        out = np.ctypeslib.as_array(args[-2], shape=(n * _ffi.NPW,)).reshape(n, _ffi.NPW)
        out[:] = np.arange(_ffi.NPW)[None, :] + 10.0 * np.arange(n)[:, None]
    monkeypatch.setattr(_ffi, "call", fake_call)
    monkeypatch.setattr(_ffi, "context", lambda *a: None)
    ev = np.zeros((2, 3, 4)); ev[0, :2, 3] = (0.25, 0.75); ev[1, 0, 3] = 0.5; ev[:, :, 1] = 1.0
    events = cj.EncounterEvents(ev, np.zeros((2, 3, 2), dtype=np.int32), np.array([2, 1], dtype=np.int32), np.zeros(2, dtype=np.int32))
    r = cj.collision_probability_window(**{**GOOD, "pairs": events, "half_window": [1.0, 2.0, 3.0], "panels": 3})
    assert seen == dict(name="mpcx_collision_probability_window", n=3, panels=3)
    assert r.pairs[:, 3].tolist() == [0.25, 0.75, 0.5]
    assert r.p.tolist() == [0.0, 10.0, 20.0] and r.start.tolist() == [1.0, 11.0, 21.0] and r.entries.tolist() == [2.0, 12.0, 22.0]
    assert r.rate_max.tolist() == [3.0, 13.0, 23.0] and r.t_rate_max.tolist() == [4.0, 14.0, 24.0]
    assert r.window.tolist() == [[5.0, 6.0], [15.0, 16.0], [25.0, 26.0]]


def collision_result(speed, sigma1):
    n = len(speed)
    out = np.zeros((n, _ffi.NPC))
    out[:, _ffi.PC_SPEED], out[:, _ffi.PC_SIGMA1], out[:, _ffi.PC_SIGMA2] = speed, sigma1, 1.0
    return cj.CollisionResult(np.zeros((n, 4)), out, np.zeros(n, dtype=np.int32))


def test_encounter_half_window():
    col = collision_result([7000.0, 0.5, 0.0, np.nan], [200.0, 100.0, 100.0, np.nan])
    h = cj.encounter_half_window(col, 10.0)
    assert h.tolist() == [(8 * 200.0 + 10.0) / 7000.0, (8 * 100.0 + 10.0) / 0.5, np.inf, np.inf]
    h = cj.encounter_half_window(col, [10.0, 20.0, 30.0, 40.0], nsigma=4)
    assert h.tolist() == [(4 * 200.0 + 10.0) / 7000.0, (4 * 100.0 + 20.0) / 0.5, np.inf, np.inf]
    for kw in (dict(col=np.zeros(4)), dict(radius_sum=[1.0, 2.0]), dict(nsigma=0.0), dict(nsigma=[8, 8, 8, 8])):
        with pytest.raises(ValueError):
            cj.encounter_half_window(**{**dict(col=col, radius_sum=10.0), **kw})
    assert cj.encounter_half_window(collision_result([], []), 1.0).shape == (0,)


def test_cumulative_probability_takes_the_window_result():
    ev = np.zeros((3, 2, 4))
    events = cj.EncounterEvents(ev, np.zeros((3, 2, 2), dtype=np.int32), np.array([2, 0, 1], dtype=np.int32), np.zeros(3, dtype=np.int32))
    out = np.zeros((3, _ffi.NPW)); out[:, _ffi.PW_P] = (0.1, 0.2, 0.5); out[:, _ffi.PW_START] = 0.9
    win = cj.WindowCollisionResult(events.events, out, np.zeros(3, dtype=np.int32))
    total = cj.cumulative_probability(events, win)
    assert np.allclose(total, [1.0 - 0.9 * 0.8, 0.0, 0.5], rtol=1e-15, atol=0.0)
    assert np.array_equal(total, cj.cumulative_probability(events, win.p))
    with pytest.raises(ValueError):
        cj.cumulative_probability(events, cj.WindowCollisionResult(events.events[:2], out[:2], np.zeros(2, dtype=np.int32)))


def test_constellation_collision_probability_window_needs_a_plan():
    from test_conjunction_host import hand_made_mpc
    mpc, _ = hand_made_mpc()
    with pytest.raises(ValueError, match="no plan"):
        mpc.collision_probability_window(1000.0, np.eye(6), 5.0, 60.0)
