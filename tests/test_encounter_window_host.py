"""The encounter window without a device: the wrapper's argument checks, the empty list, ConstellationMPC's half_window='auto'
keywords, and the restatement (encounter_window_reference.py) against a closed form of its own."""
import numpy as np
import pytest

import encounter_window_reference as E


def small_side(S=2, K=5):
    Y, units, span = np.zeros((S, 7, K)), np.ones((S, 2)), np.array([[0.0, 1.0]] * S)
    return Y, units, span, np.zeros((S, K, 6, 6))


@pytest.fixture
def no_library_call(monkeypatch):
    from mpconstellation_amd import _ffi

    def refuse(*a, **k):
        raise AssertionError("a library call was made")
    monkeypatch.setattr(_ffi, "call", refuse)


def test_wrapper_refuses_bad_arguments(no_library_call):
    from mpconstellation_amd import encounter_window
    Y, units, span, P = small_side()
    pairs = np.zeros((3, 4))
    ok = dict(pairs=pairs, radius=1.0, Y=Y, units=units, span=span, P=P, max_half=10.0)
    for bad, word in ((dict(pairs=np.zeros((3, 5))), "pairs"), (dict(pairs=np.zeros(4)), "pairs"), (dict(P=P[:, :4]), "P:"), (dict(P=None), "P and radius"),
                      (dict(Y=Y[:, :6]), "Y:"), (dict(units=units[:1]), "units"), (dict(span=span[:1]), "span"), (dict(radius=np.ones(3)), "radius"),
                      (dict(max_half=np.ones(2)), "max_half"), (dict(max_half=np.ones((3, 1))), "max_half"), (dict(max_half=None), "max_half"),
                      (dict(nsigma=0.0), "nsigma"), (dict(nsigma=-8.0), "nsigma"), (dict(nsigma=np.nan), "nsigma"), (dict(nsigma=np.inf), "nsigma"),
                      (dict(nsigma=[8.0]), "nsigma"), (dict(nsigma="8"), "nsigma"), (dict(levels=0), "levels"), (dict(levels=5), "levels"),
                      (dict(levels=1.5), "levels"), (dict(levels=[3]), "levels"), (dict(mu=0.0), "mu"),
                      (dict(cat=(Y, units, span, P)), "cat"), (dict(cat=(Y, units, span, P, 1.0, None, None)), "cat"),
                      (dict(cat=(Y, units, span, P[:1], 1.0)), "cat_P")):
        with pytest.raises(ValueError, match=word):
            encounter_window(**{**ok, **bad})


def test_empty_list_makes_no_library_call(no_library_call):
    from mpconstellation_amd import encounter_window, EncounterWindowResult
    Y, units, span, P = small_side()
    res = encounter_window(np.empty((0, 4)), 1.0, Y, units, span, P, 10.0)
    assert isinstance(res, EncounterWindowResult) and res.pairs.shape == (0, 4)
    assert res.half.shape == (0,) and res.window.shape == (0, 2) and res.reach.shape == (0, 2) and res.g0.shape == (0,)
    assert res.flags.shape == (0,) and res.flags.dtype == np.int32 and res.status.shape == (0,) and res.status.dtype == np.int32
    assert res.clear.shape == (0,) and res.open.shape == (0, 2)
    assert encounter_window(np.empty((0, 4)), 1.0, Y, units, span, P, np.empty(0), cat=(Y, units, span, P, 2.0)).half.shape == (0,)


def test_result_reads_its_flags():
    from mpconstellation_amd import EncounterWindowResult, _ffi
    out = np.arange(4.0 * _ffi.NEW).reshape(4, _ffi.NEW)
    r = EncounterWindowResult(np.zeros((4, 4)), out, np.array([0, 1, 6, 12], dtype=np.int32), np.zeros(4, dtype=np.int32))
    assert r.clear.tolist() == [False, True, False, False] and r.open.tolist() == [[False, False], [False, False], [True, True], [False, True]]
    assert np.array_equal(r.half, out[:, 0]) and np.array_equal(r.window, out[:, 1:3]) and np.array_equal(r.reach, out[:, 3:5]) and np.array_equal(r.g0, out[:, 5])
    assert (_ffi.NEW, _ffi.EW_MAX_LEVELS) == (E.NEW, E.MAX_LEVELS) and (_ffi.EW_CLEAR, _ffi.EW_OPEN_BEFORE, _ffi.EW_OPEN_AFTER, _ffi.EW_BAD_SCAN) == (1, 2, 4, 8)


def test_constellation_mpc_auto_keywords_are_tested_before_anything_runs(no_library_call):
    """'auto' with a bad max_half or nsigma, any other string, and max_half beside a number raise -- before the plan is looked at
    (there is none here) and without a library call"""
    from mpconstellation_amd import Satellite, ConstellationMPC
    from mpconstellation_amd.constellation import constellation_states
    mpc = ConstellationMPC([Satellite(s[:3].copy(), s[3:6].copy(), float(s[6])) for s in constellation_states(3)], base_res=30)
    P0 = np.eye(6)
    calls = (lambda h, **kw: mpc.collision_probability_window(1000.0, P0, 5.0, h, **kw),
             lambda h, **kw: mpc.collision_probability_mc(1000.0, P0, 5.0, h, 16, **kw),
             lambda h, **kw: mpc.avoidance_window(1000.0, P0, 5.0, h, 1e-6, **kw),
             lambda h, **kw: mpc.avoidance_window_refine(1000.0, P0, 5.0, h, 1e-6, **kw))
    for call in calls:
        for mh in (0.0, -1.0, np.nan, np.inf, [10.0, -1.0], np.ones((2, 2)), "wide"):
            with pytest.raises(ValueError, match="max_half"):
                call("auto", max_half=mh)
        for ns in (0.0, -8.0, np.nan, np.inf, [8.0], "8"):
            with pytest.raises(ValueError, match="nsigma"):
                call("auto", nsigma=ns)
        for word in ("Auto", "automatic", ""):
            with pytest.raises(ValueError, match="half_window"):
                call(word)
        with pytest.raises(ValueError, match="max_half"):
            call(60.0, max_half=100.0)
        with pytest.raises(ValueError, match="no plan yet"):                # well-formed: the method goes on to the plan
            call("auto", max_half=100.0, nsigma=6.0)
        with pytest.raises(ValueError, match="no plan yet"):
            call(60.0)
    with pytest.raises(TypeError):
        mpc.collision_probability_window(1000.0, P0, 5.0, "auto", 4, None, 4, None, None, None, None, 100.0)      # (keyword-only)


def straight_line(d0, speed, sigma, R, nsigma, span=np.inf, bad_from=np.inf):
    """g of window_search for a relative motion on a straight line at `speed` past the miss d0, an isotropic constant sigma: d = (d0,
    speed offset, 0), L^-1 = I / sigma; outside [-span, span]: ST_BADK; from the offset bad_from on: ST_NUMERIC"""
    def g(sg, off):
        d = np.array([np.full(len(off), d0), sg * speed * off, np.zeros(len(off))])
        i, z = np.full(len(off), 1.0 / sigma), np.zeros(len(off))
        gv = E.g_of(d, (i, z, i, z, z, i), R, nsigma)
        code = np.where(off > span, E.ST_BADK, np.where(off >= bad_from, E.ST_NUMERIC, E.ST_OK))
        return code, np.where(code == E.ST_OK, gv, np.nan)
    return g


@pytest.mark.parametrize("levels", [1, 2, 3, 4])
def test_reference_brackets_the_closed_form(levels):
    """|L^-1 d| = sqrt(d0^2 + (speed h)^2) / sigma and |L^-1|_F = sqrt(3) / sigma: g = 0 at h* = sqrt((nsigma sigma + sqrt(3) R)^2 -
    d0^2) / speed.  The reach is the end of the final cell that holds h*: h* <= reach <= h* + H / 64^levels (a relative 1e-12 for the
    rounding of g at the cell ends)."""
    for d0, speed, sigma, R, nsigma, H in ((300.0, 8500.0, 282.84, 20.0, 8.0, 600.0), (0.0, 0.15, 150.0, 25.0, 8.0, 20000.0),
                                           (900.0, 2.0, 100.0, 0.0, 10.0, 777.0), (50.0, 40.0, 500.0, -3.0, 3.0, 1000.0)):
        hs = np.sqrt((nsigma * sigma + np.sqrt(3.0) * max(R, 0.0)) ** 2 - d0 ** 2) / speed
        assert hs < H
        st, reach, g0, flags, margin = E.window_search(straight_line(d0, speed, sigma, max(R, 0.0), nsigma), H, levels)
        cell = H / 64.0 ** levels
        assert st == E.ST_OK and flags == 0 and g0 < 0.0 and margin > 0.0
        assert g0 == pytest.approx(d0 / sigma - np.sqrt(3.0) * max(R, 0.0) / sigma - nsigma, abs=1e-12)
        for r in reach:
            assert hs * (1.0 - 1e-12) <= r <= hs * (1.0 + 1e-12) + cell, (d0, speed, levels, r, hs, cell)
        assert reach[0] == reach[1]


def test_reference_flags_follow_g_and_max_half():
    sigma, R, nsigma, speed = 100.0, 10.0, 8.0, 1.0
    live_to = (nsigma * sigma + np.sqrt(3.0) * R) / speed                  # h* of a central pass: 817.3 s
    # open: max_half ends before the live stretch does -- the reach is max_half itself, at every level count
    for levels in (1, 3):
        st, reach, g0, flags, _ = E.window_search(straight_line(0.0, speed, sigma, R, nsigma), 500.0, levels)
        assert (st, reach, flags) == (E.ST_OK, [500.0, 500.0], E.OPEN_BEFORE | E.OPEN_AFTER)
    # closed as soon as max_half passes it
    st, reach, g0, flags, _ = E.window_search(straight_line(0.0, speed, sigma, R, nsigma), 1000.0, 2)
    assert flags == 0 and live_to <= reach[0] <= live_to + 1000.0 / 64.0 ** 2
    # clear: g(t) > 0 -- both reaches one final cell, nothing searched (a g that fails beyond t is never asked)
    for levels in (1, 2, 3, 4):
        st, reach, g0, flags, margin = E.window_search(straight_line(1000.0, speed, sigma, R, nsigma, bad_from=1e-9), 640.0, levels)
        assert (st, flags) == (E.ST_OK, E.CLEAR) and reach == [640.0 / 64.0 ** levels] * 2 and g0 > 0.0 and margin == g0
    # a span end inside the live stretch closes the side without an open flag: at most the distance to it plus one final cell
    st, reach, g0, flags, _ = E.window_search(straight_line(0.0, speed, sigma, R, nsigma, span=333.0), 2000.0, 3)
    assert flags == 0 and 333.0 < reach[0] <= 333.0 + 2000.0 / 64.0 ** 3 and reach[0] == reach[1]
    # a numerically bad scan time counts as live and sets its flag; here every time from 700 s on: the side is open
    st, reach, g0, flags, _ = E.window_search(straight_line(0.0, speed, sigma, R, nsigma, bad_from=700.0), 2000.0, 3)
    assert st == E.ST_OK and flags == E.BAD_SCAN | E.OPEN_BEFORE | E.OPEN_AFTER and reach == [2000.0, 2000.0]
    # the row's own time failing is the row's status
    st, reach, g0, flags, _ = E.window_search(straight_line(0.0, speed, sigma, R, nsigma, bad_from=0.0), 2000.0, 3)
    assert st == E.ST_NUMERIC and reach is None and flags == 0
    st, reach, g0, flags, _ = E.window_search(straight_line(np.inf, speed, sigma, R, nsigma), 2000.0, 3)
    assert st == E.ST_NUMERIC


def test_reference_on_trajectories_has_the_documented_statuses():
    """the full path on a small scene: max_half 0, negative, NaN, inf and a bad index are ST_BADK, a radius that is not finite
    ST_NUMERIC, each NaN with flags 0; a good row is untouched by them"""
    import collision_window_reference as W
    sc = W.window_scene(3)
    pairs = sc["pairs"][:8].copy()
    H = np.array([400.0, 0.0, -1.0, np.nan, np.inf, 400.0, 400.0, 400.0])
    pairs[5, 0] = 99.0
    Y, units, span, P, radius, ns = sc["rows"]
    cat = list(sc["cat"]); cat[4] = cat[4].copy(); cat[4][6] = np.nan
    out, flags, status, margin = E.encounter_window(pairs, sc["rows"], H, 8.0, 3, tuple(cat))
    B, N = E.ST_BADK, E.ST_NUMERIC
    assert status.tolist() == [0, B, B, B, B, B, N, 0]
    assert np.isnan(out[status != 0]).all() and (flags[status != 0] == 0).all() and np.isfinite(out[status == 0]).all()
    alone = E.encounter_window(pairs[7:8], sc["rows"], 400.0, 8.0, 3, sc["cat"])
    assert np.array_equal(alone[0][0], out[7]) and alone[1][0] == flags[7] and alone[3][0] == margin[7]
