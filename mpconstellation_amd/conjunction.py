"""Conjunction screening: the constellation on one clock, and the closest approach of every pair of satellites on it.

Everything else in the package works on one satellite in its own units (SatelliteScale: length = its start radius, time = its
own orbital period), so node k of two trajectories is two different instants in two different lengths, and nothing looks at two
satellites at once.  Here (include/mpcx.h, csrc/conjunction.hip: one screen kernel and one host path behind both screens):

  common_clock   resamples trajectories at M common instants in metres and m/s (cubic Hermite on the node positions and velocities);
  screen         the closest approach of every ordered pair over every grid interval -- per satellite the nearest other one, how
                 near and when, and with a threshold the list of pairs that come closer than it;
  screen_against the same for a constellation against a catalogue of foreign objects (debris, other operators' satellites): the
                 rectangle satellites x objects, not the square of the union;
  screen_pairs   the closest approach of the pairs of a list alone, with the bits the screens give them;
  screen_events  EVERY close approach of the listed pairs below a threshold (a window of several revolutions holds about two per
                 revolution), as rows that every call below takes; cumulative_probability joins their probabilities per pair;
  screen_track   of those close approaches the one nearest each listed row's own time: an encounter followed through re-screens;
  catalogue_trajectories   a catalogue given as state vectors at an epoch, propagated to trajectories for screen_against;
  covariance     a position / velocity covariance propagated along trajectories by the state-transition matrices of the linearisation;
  covariance_thrust   the same with the execution errors of the thrust (the Gates model; gates_execution turns newtons into its
                 figures): all seven states and both input blocks of the linearisation, for the covariance after a burn;
  covariance_drag     covariance_thrust with an uncertain drag: a Gauss-Markov scale error on density times ballistic coefficient as
                 an eighth state, driven by the drag column of the linearisation, for predictions over several revolutions;
  collision_probability   for every pair a screen lists, the short-encounter collision probability in the encounter plane;
  collision_probability_window   for encounters too slow for that model (neighbours in one shell, satellites deployed together):
                 the probability over a time window from the time-varying relative state and the full 6 x 6 covariances;
                 encounter_half_window is the window inside which the two models must agree;
  encounter_window   that window chosen on the device for every listed row, fast or without any relative speed: the stretch of time
                 about the row's time within nsigma combined sigmas of a collision;
  collision_probability_mc   the same rows by sampled flights through the nonlinear dynamics: initial states, masses and thrust
                 execution errors drawn, flown and counted -- what the linearised figures above are held against;
  catalogue_covariance    catalogue_trajectories followed by covariance;
  avoidance      for every listed pair the derivative of the encounter-plane miss with respect to every thrust node of the plan, and
                 the least-effort thrust change that opens the miss to a requested distance.
  avoidance_joint   per manoeuvring satellite ONE thrust change that opens all of its listed encounters at once, inside its thrust
                 limit, and optionally holds the plan's terminal state.
  avoidance_refine  that manoeuvre flown through the nonlinear dynamics, re-screened, linearised and corrected, a fixed number of
                 rounds on the device: the answer as flown; with track=True every row follows its own encounter (screen_track), which
                 a list of screen_events' rows needs.

The device does all of it (4096 satellites are 8.4 M pairs times the grid); there is no host path."""
import numpy as np

from . import _ffi
from .linearize_discretize import Discretizer
from .sharding import dispatch

DEFAULT_MAX_PAIRS = 65536


class ConjunctionResult:
    """dmin (S,) metres, partner (S,) int32 (-1: none), tca (S,) seconds: each satellite's closest approach to any other one.
    pairs (n, 4) float64 rows (i, j, distance, time) with i < j, sorted by (i, j): the pairs at or below the threshold -- at most
    max_pairs of them; n_pairs_total is how many there are.  status (S,) int32 or None: the ephemeris' MPCX_ST_* per satellite
    when the screen started from trajectories.
    From screen_against: partner indexes the catalogue, pairs rows are (satellite, catalogue object, distance, time) -- any i, j --
    and cat_status (D,) is the catalogue's ephemeris status (None from ephemerides)."""

    def __init__(self, dmin, partner, tca, pairs, n_pairs_total, status=None, cat_status=None):
        self.dmin, self.partner, self.tca, self.pairs, self.n_pairs_total, self.status = dmin, partner, tca, pairs, int(n_pairs_total), status
        self.cat_status = cat_status

    def __repr__(self):
        return f"ConjunctionResult(S={len(self.dmin)}, pairs={len(self.pairs)} of {self.n_pairs_total})"


def sort_pairs(pairs):
    """rows (i, j, d, t) sorted by (i, j)"""
    pairs = np.asarray(pairs, dtype=np.float64).reshape(-1, 4)
    return pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]


def _check_grid(M, T0, T1):
    if int(M) != M or M < 2:
        raise ValueError(f"M: need an integer >= 2 common instants, got {M}")
    if not (np.isfinite(T0) and np.isfinite(T1) and T1 > T0):
        raise ValueError(f"need finite T0 < T1, got [{T0}, {T1}]")
    return int(M), float(T0), float(T1)


def _check_trajectories(Y, units, span, ns, pre=""):
    """pre: the prefix of the argument names in the messages ('cat_' for a catalogue's)"""
    Y = _ffi.as_f64(Y)
    if Y.ndim != 3 or Y.shape[1] != 7 or Y.shape[0] < 1 or Y.shape[2] < 1:
        raise ValueError(f"{pre}Y: expected (S, 7, n) normalised trajectories, got {Y.shape}")
    S = Y.shape[0]
    if units is None or span is None:
        raise ValueError(f"{pre}units and {pre}span are required with {pre}Y")
    units, span = _ffi.as_f64(units), _ffi.as_f64(span)
    if units.shape != (S, 2):
        raise ValueError(f"{pre}units: expected ({S}, 2) = (length unit in m, time unit in s) per satellite, got {units.shape}")
    if span.shape != (S, 2):
        raise ValueError(f"{pre}span: expected ({S}, 2) = physical times of the first and last node per satellite, got {span.shape}")
    if ns is not None and np.shape(ns) != (S,):
        raise ValueError(f"{pre}ns: expected ({S},) node counts, got {np.shape(ns)}")
    return Y, units, span, _ffi.counts(ns, S)


# ---- the checks and the marshalling that the calls below share
def _as_pairs(pairs):
    """the list of a call: (n, 4) rows, a ConjunctionResult (its .pairs) or an EncounterEvents (its .events)"""
    if isinstance(pairs, ConjunctionResult):
        pairs = pairs.pairs
    elif isinstance(pairs, EncounterEvents):
        pairs = pairs.events
    pairs = _ffi.as_f64(pairs)
    if pairs.ndim != 2 or pairs.shape[1] != 4:
        raise ValueError(f"pairs: expected (n, 4) rows (i, j, distance, time), a ConjunctionResult or an EncounterEvents, got {pairs.shape}")
    return pairs


def _per_row(v, N, name, what):
    """a scalar or (N,) argument `name` (its values are `what` in the message) as the (N,) float64 array the library takes"""
    if v is None or np.ndim(v) not in (0, 1) or (np.ndim(v) == 1 and np.shape(v) != (N,)):
        raise ValueError(f"{name}: expected a scalar or ({N},) {what}, got {None if v is None else np.shape(v)}")
    return _ffi.per_sat(v, N)


def _check_mu(mu):
    from .constants import MU_EARTH
    mu = float(MU_EARTH if mu is None else mu)
    if not mu > 0.0:
        raise ValueError(f"mu: need > 0 m^3/s^2, got {mu}")
    return mu


def _model(include_drag, include_J2, atmosphere, max_step):
    """the model of a linearisation as the block functions take it: the keywords flags, max_step and atmosphere"""
    if not max_step > 0.0:
        raise ValueError(f"max_step: need > 0, got {max_step}")
    return dict(flags=_ffi.model_flags(include_drag, include_J2, atmosphere), max_step=float(max_step), atmosphere=atmosphere)


def _context(device, slot, flags=0, atmosphere=None):
    """context (device, slot), given the atmosphere first when the flags carry FLAG_ATMO"""
    return _ffi.atmosphere_context(device, slot, atmosphere if flags & _ffi.FLAG_ATMO else None)


def _side_args(side, extras=0):
    """one side of a call as the library takes it: count, row length, ns, Y, units, span and `extras` more pointers.  side =
    (Y, units, span, ns) of _check_trajectories (extras 0), (Y, units, span, ns, P) of _check_cat (1: the covariances) or (Y, units,
    span, P, radius, ns) of _check_side (2: the covariances and the radii); None: the side is absent"""
    if side is None:
        return (0, 0, None, None, None, None) + (None,) * extras
    Y, units, span = side[:3]
    ns, rest = (side[5], side[3:5]) if extras == 2 else (side[3], side[4:])
    return (Y.shape[0], Y.shape[2], _ffi.iptr_opt(ns), _ffi.dptr(Y), _ffi.dptr(units), _ffi.dptr(span), *[_ffi.dptr_opt(a) for a in rest])


def common_clock(Y, units, span, M, T0, T1, ns=None, device=0, return_status=False):
    """Y (S, 7, n) normalised trajectories (ns (S,): nodes in use per satellite, None: all n), units (S, 2) each satellite's length
    unit (m) and time unit (s), span (S, 2) the physical times (s) of its first and last node (uniform in between) -> eph (S, 6, M):
    position (m) and velocity (m/s) at linspace(T0, T1, M).  Instants outside a satellite's span are NaN; a satellite with fewer than
    two nodes or an empty span is NaN throughout (status MPCX_ST_BADK = 9; return_status=True returns (eph, status))."""
    M, T0, T1 = _check_grid(M, T0, T1)
    Y, units, span, ns = _check_trajectories(Y, units, span, ns)
    S, _, n = Y.shape
    eph = _ffi.result_pool.take((S, 6, M))
    status = np.zeros(S, dtype=np.int32)
    _ffi.call("mpcx_ephemeris_batch", _ffi.context(device), S, n, _ffi.iptr_opt(ns), _ffi.dptr(Y), _ffi.dptr(units), _ffi.dptr(span), M, T0, T1,
              _ffi.dptr(eph), _ffi.iptr(status))
    return (eph, status) if return_status else eph


def _check_options(who, T0, T1, threshold, max_pairs):
    """the options screen and screen_against share -> the threshold as the library takes it (0.0: no list)"""
    if T0 is None or T1 is None:
        raise ValueError(f"{who}: T0 and T1 (the common grid's first and last instant, seconds) are required")
    if int(max_pairs) != max_pairs or max_pairs < 0:
        raise ValueError(f"max_pairs: need an integer >= 0, got {max_pairs}")
    thr = 0.0 if threshold is None else float(threshold)
    if not thr == thr:
        raise ValueError("threshold is NaN")
    return thr


def _check_ephemeris(eph, M, name="eph", count="S"):
    """an (N, 6, M) ephemeris argument; M: what the caller gave beside it, or None"""
    eph = _ffi.as_f64(eph)
    if eph.ndim != 3 or eph.shape[1] != 6 or eph.shape[0] < 1:
        raise ValueError(f"{name}: expected ({count}, 6, M), got {eph.shape}")
    if M is not None and int(M) != eph.shape[2]:
        raise ValueError(f"M = {M} but {name} has {eph.shape[2]} instants")
    return eph


def screen(eph=None, T0=None, T1=None, threshold=None, max_pairs=DEFAULT_MAX_PAIRS, device=0, devices=None, *, Y=None, units=None,
           span=None, ns=None, M=None):
    """The closest approach of every pair on the common grid linspace(T0, T1, M).  Either eph (S, 6, M) from common_clock, or the
    trajectories Y, units, span [, ns] and M (the fused call: the ephemeris never leaves the device).  threshold (metres; None or
    <= 0: no list) and max_pairs: ConjunctionResult.pairs.  devices=[d0, d1, ...]: contiguous blocks of ROWS on several devices
    (sharding.sharded_call); every device holds the whole ephemeris, results are written in place, the bits are those of one device."""
    if (eph is None) == (Y is None):
        raise ValueError("screen: give either eph or the trajectories Y, units, span, M")
    thr = _check_options("screen", T0, T1, threshold, max_pairs)
    if eph is not None:
        eph = _check_ephemeris(eph, M)
        src, M = (eph,), eph.shape[2]
    else:
        if M is None:
            raise ValueError("screen: M (the number of common instants) is required with trajectories")
        src = _check_trajectories(Y, units, span, ns)
    return _screen(src, None, M, T0, T1, thr, max_pairs, device, devices)


def screen_against(eph=None, cat_eph=None, T0=None, T1=None, threshold=None, max_pairs=DEFAULT_MAX_PAIRS, device=0, devices=None, *,
                   Y=None, units=None, span=None, ns=None, cat_Y=None, cat_units=None, cat_span=None, cat_ns=None, M=None):
    """The closest approach of every satellite of a constellation to any object of a foreign catalogue on the common grid
    linspace(T0, T1, M): S x D pairs, not the (S + D)^2 of screening the union.  Both sides in the same form: either eph (S, 6, M)
    and cat_eph (D, 6, M) from common_clock with the same M, T0, T1, or the trajectories Y, units, span [, ns] and cat_Y, cat_units,
    cat_span [, cat_ns] with M (the fused call: neither ephemeris leaves the device; the catalogue has its own node count, units
    and spans).  Returns a ConjunctionResult whose partner indexes the catalogue and whose pairs rows are (satellite, catalogue
    object, distance, time), sorted by (i, j); status and cat_status are the two ephemerides' (None from ephemerides).  The bits of
    a pair are those screen gives it in the union [constellation; catalogue].  devices=[d0, d1, ...]: contiguous blocks of ROWS on
    several devices (sharding.sharded_call); every device holds the whole catalogue, the bits are those of one device."""
    given_eph, given_traj = eph is not None or cat_eph is not None, Y is not None or cat_Y is not None
    if given_eph and given_traj:
        raise ValueError("screen_against: constellation and catalogue must come in the same form, both ephemerides or both "
                         "trajectories; put the one given as trajectories on the grid with common_clock first")
    if given_eph == given_traj:
        raise ValueError("screen_against: give either eph and cat_eph, or the trajectories Y, units, span and cat_Y, cat_units, cat_span with M")
    thr = _check_options("screen_against", T0, T1, threshold, max_pairs)
    if given_eph:
        if eph is None or cat_eph is None:
            raise ValueError("screen_against: eph and cat_eph are both required")
        eph, cat_eph = _check_ephemeris(eph, M), _check_ephemeris(cat_eph, None, "cat_eph", "D")
        if cat_eph.shape[2] != eph.shape[2]:
            raise ValueError(f"eph has {eph.shape[2]} instants but cat_eph {cat_eph.shape[2]}: both must be on the same grid")
        src, cat, M = (eph,), (cat_eph,), eph.shape[2]
    else:
        if Y is None or cat_Y is None:
            raise ValueError("screen_against: Y and cat_Y are both required")
        if M is None:
            raise ValueError("screen_against: M (the number of common instants) is required with trajectories")
        src, cat = _check_trajectories(Y, units, span, ns), _check_trajectories(cat_Y, cat_units, cat_span, cat_ns, "cat_")
    return _screen(src, cat, M, T0, T1, thr, max_pairs, device, devices)


def _screen(src, cat, M, T0, T1, thr, max_pairs, device, devices):
    """Both screens behind their argument checks.  src, cat: the rows' and the columns' side, each (eph,) or (Y, units, span, ns);
    cat None: all pairs of src.  Blocks of rows go to the devices, their lists are joined and sorted."""
    M, T0, T1 = _check_grid(M, T0, T1)
    S = src[0].shape[0]
    out = dict(dmin=np.empty(S), partner=np.empty(S, dtype=np.int32), tca=np.empty(S))
    how = dict(src=src, cat=cat, M=M, T0=T0, T1=T1, thr=thr, max_pairs=int(max_pairs) if thr > 0.0 else 0)
    parts = dispatch(_screen_call, [np.arange(S)], out, device, devices, **how)
    pairs = sort_pairs(np.concatenate([p for p, _, _ in parts]))[:int(max_pairs)]
    return ConjunctionResult(out["dmin"], out["partner"], out["tca"], pairs, sum(n for _, n, _ in parts), *parts[0][2])


def _screen_call(rows, *, device, slot, out, src, cat, M, T0, T1, thr, max_pairs):
    """One block of rows against all columns on context (device, slot): dmin, partner, tca into `out` (the block's views); returns
    the block's pairs (all pairs: those whose smaller index is one of its rows), how many there are, and the ephemeris statuses
    (status, cat_status) of the fused calls, None where there is none."""
    row0, nrows = int(rows[0]), len(rows)
    pairs = np.zeros((max_pairs, 4))
    n_pairs = np.zeros(1, dtype=np.int64)
    tail = (T0, T1, row0, nrows, thr, max_pairs, _ffi.dptr(out["dmin"]), _ffi.iptr(out["partner"]), _ffi.dptr(out["tca"]), _ffi.dptr(pairs),
            n_pairs.ctypes.data_as(_ffi._lp))
    ctx = _ffi.context(device, slot)
    name, sides = ("mpcx_conjunction_screen", [src]) if cat is None else ("mpcx_conjunction_cross_screen", [src, cat])
    counts = [side[0].shape[0] for side in sides]                    # S [, D]
    statuses = [None, None]
    if len(src) == 1:
        _ffi.call(name, ctx, *counts, M, *[_ffi.dptr(eph) for eph, in sides], *tail)
    else:
        statuses[:len(sides)] = [np.zeros(N, dtype=np.int32) for N in counts]
        _ffi.call(name + "_traj", ctx, *[a for side in sides for a in _side_args(side)], M, *tail, *[_ffi.iptr(st) for st in statuses[:len(sides)]])
    n = int(n_pairs[0])
    return pairs[:min(n, max_pairs)], n, statuses


def _check_list_call(who, pairs, T0, T1, eph, cat_eph, Y, units, span, ns, cat_Y, cat_units, cat_span, cat_ns, M):
    """the checks screen_pairs and screen_events make of the list, the two sides and the grid -> (pairs, src, cat, M, T0, T1,
    given_traj); src, cat: each side as (eph,) or (Y, units, span, ns), cat None without a catalogue"""
    pairs = _as_pairs(pairs)
    given_eph, given_traj = eph is not None or cat_eph is not None, Y is not None or cat_Y is not None
    if given_eph == given_traj:
        raise ValueError(f"{who}: give either eph [, cat_eph], or the trajectories Y, units, span [, cat_Y, cat_units, cat_span] with M")
    if T0 is None or T1 is None:
        raise ValueError(f"{who}: T0 and T1 (the common grid's first and last instant, seconds) are required")
    cat = None
    if given_eph:
        if eph is None:
            raise ValueError(f"{who}: cat_eph needs eph")
        eph = _check_ephemeris(eph, M)
        src, M = (eph,), eph.shape[2]
        if cat_eph is not None:
            cat_eph = _check_ephemeris(cat_eph, None, "cat_eph", "D")
            if cat_eph.shape[2] != M:
                raise ValueError(f"eph has {M} instants but cat_eph {cat_eph.shape[2]}: both must be on the same grid")
            cat = (cat_eph,)
    else:
        if Y is None:
            raise ValueError(f"{who}: cat_Y needs Y")
        if M is None:
            raise ValueError(f"{who}: M (the number of common instants) is required with trajectories")
        src = _check_trajectories(Y, units, span, ns)
        if cat_Y is not None:
            cat = _check_trajectories(cat_Y, cat_units, cat_span, cat_ns, "cat_")
    M, T0, T1 = _check_grid(M, T0, T1)
    return pairs, src, cat, M, T0, T1, given_traj


def screen_pairs(pairs, T0, T1, eph=None, cat_eph=None, device=0, devices=None, *, Y=None, units=None, span=None, ns=None, cat_Y=None,
                 cat_units=None, cat_span=None, cat_ns=None, M=None):
    """The closest approach of the LISTED pairs alone on the common grid linspace(T0, T1, M): n x M work where the screens do
    S^2 x M -- a screen's list looked at again after the trajectories changed.  pairs: (n, 4) rows (i, j, ., .) as screen and
    screen_against list them, or their ConjunctionResult; only i and j are read.  Both sides as the screens take them: eph [,
    cat_eph], or the trajectories Y, units, span [, ns] [and cat_Y, cat_units, cat_span [, cat_ns]] with M.  With a catalogue j
    indexes it; without one j indexes the constellation and either order of (i, j) is accepted.  Returns (out, status): out (n, 4)
    rows (i, j, distance, time) in list order -- (+inf, NaN) for a pair without a common valid interval -- and status (n,) int32,
    MPCX_ST_BADK = 9 with NaN distance and time for an index outside its side or i == j.  From trajectories it returns (out, status,
    eph_status, cat_status), the ephemerides' statuses as the screens return them (cat_status None without a catalogue).  Distance
    and time of a pair are bit for bit what screen / screen_against list for it on the same inputs.  An empty list returns empty
    arrays without a library call.  devices=[d0, d1, ...]: contiguous blocks of the list's rows on several devices (every device
    holds both sides), written in place, the bits of one device."""
    pairs, src, cat, M, T0, T1, given_traj = _check_list_call("screen_pairs", pairs, T0, T1, eph, cat_eph, Y, units, span, ns, cat_Y, cat_units,
                                                              cat_span, cat_ns, M)
    n = pairs.shape[0]
    out = dict(out=np.empty((n, 4)), status=np.zeros(n, dtype=np.int32))
    statuses = _screen_list(pairs, out, device, devices, src=src, cat=cat, M=M, T0=T0, T1=T1)
    return (out["out"], out["status"], *statuses) if given_traj else (out["out"], out["status"])


def _screen_list(pairs, out, device, devices, **how):
    """the blocks of a list's rows to the devices -> the ephemeris statuses of the first; an empty list makes no call and has none"""
    if not len(pairs):
        return [None, None]
    return dispatch(_screen_pairs_call, [pairs], out, device, devices, **how)[0]


def _screen_pairs_call(pairs, *, device, slot, out, src, cat, M, T0, T1, events=None, track=None):
    """one block of the list's rows on context (device, slot), into `out` (the block's views); returns the ephemeris statuses
    [status, cat_status] of the calls from trajectories, None where there is none.  events = (threshold, max_events): every close
    approach (mpcx_conjunction_events*) into out's events, info, count and status instead of the closest one into out and status;
    track = max_shift: the close approach nearest each row's time (mpcx_conjunction_track*) into out's out, info and status"""
    pairs = _ffi.as_f64(pairs)
    ctx = _ffi.context(device, slot)
    S, D = src[0].shape[0], 0 if cat is None else cat[0].shape[0]
    if track is not None:
        name, tail = "mpcx_conjunction_track", (T0, T1, track, _ffi.dptr(out["out"]), _ffi.iptr(out["info"]), _ffi.iptr(out["status"]))
    elif events is None:
        name, tail = "mpcx_conjunction_pairs", (T0, T1, _ffi.dptr(out["out"]), _ffi.iptr(out["status"]))
    else:
        name, tail = "mpcx_conjunction_events", (T0, T1, *events, _ffi.dptr(out["events"]), _ffi.iptr(out["info"]), _ffi.iptr(out["count"]),
                                                 _ffi.iptr(out["status"]))
    if len(src) == 1:
        _ffi.call(name, ctx, len(pairs), _ffi.dptr(pairs), S, D, M, _ffi.dptr(src[0]),
                  _ffi.dptr_opt(None if cat is None else cat[0]), *tail)
        return [None, None]
    statuses = [np.zeros(S, dtype=np.int32), None if cat is None else np.zeros(D, dtype=np.int32)]
    _ffi.call(name + "_traj", ctx, len(pairs), _ffi.dptr(pairs), *_side_args(src), *_side_args(cat), M, *tail,
              *[_ffi.iptr_opt(st) for st in statuses])
    return statuses


DEFAULT_MAX_EVENTS = 16


class EncounterEvents:
    """Every close approach of the n pairs of a list (screen_events).  Per stored event, list order first, then time: events (n_ev, 4)
    rows (i, j, distance in m, time in s) -- a valid `pairs` argument for collision_probability, avoidance, avoidance_joint and
    screen_pairs, which treat every row on its own with the row's time as the encounter --, row (n_ev,) the list row the event
    belongs to, interval (n_ev,) its grid interval, edge (n_ev,) bool: the distance is still falling where the pair's common
    span ends.  Per list row: count (n,) the events found, truncated (n,) bool count > max_events (the earliest max_events are
    stored), status (n,) int32 MPCX_ST_* (9: an index outside its side or i == j; count 0).  eph_status, cat_status: the
    ephemerides' statuses from trajectories, else None."""

    def __init__(self, events, info, count, status, eph_status=None, cat_status=None):
        """from the library's padded blocks: events (n, E, 4), info (n, E, 2), count (n,), status (n,)"""
        events, info, count = np.asarray(events, dtype=np.float64), np.asarray(info, dtype=np.int32), np.asarray(count, dtype=np.int32)
        if events.ndim != 3 or events.shape[2] != 4 or info.shape != events.shape[:2] + (2,) or count.shape != events.shape[:1]:
            raise ValueError(f"expected events (n, E, 4), info (n, E, 2) and count (n,), got {events.shape}, {info.shape}, {count.shape}")
        n, E = events.shape[:2]
        stored = np.arange(E)[None, :] < np.minimum(count, E)[:, None]   # (n, E): row-major, so list order first, then slot = time
        self.max_events = E
        self.events = np.ascontiguousarray(events[stored]).reshape(-1, 4)
        self.row = np.nonzero(stored)[0]
        self.interval, self.edge = info[stored][:, 0], info[stored][:, 1] != 0
        self.count, self.truncated, self.status = count, count > E, np.asarray(status, dtype=np.int32)
        self.eph_status, self.cat_status = eph_status, cat_status

    def __repr__(self):
        return f"EncounterEvents(pairs={len(self.count)}, events={len(self.events)} of {int(self.count.sum())})"


def screen_events(pairs, T0, T1, threshold=None, max_events=DEFAULT_MAX_EVENTS, eph=None, cat_eph=None, device=0, devices=None, *, Y=None,
                  units=None, span=None, ns=None, cat_Y=None, cat_units=None, cat_span=None, cat_ns=None, M=None):
    """EVERY close approach of the listed pairs on the common grid linspace(T0, T1, M) -> EncounterEvents.  screen_pairs returns a
    pair's global minimum, which is the only one in a window shorter than an orbit; over several revolutions two objects on crossing
    orbits come close about twice per revolution.  An event is a local minimum of the per-interval closest approach over the grid
    (include/mpcx.h: mpcx_conjunction_events); threshold (metres; None or <= 0: every event) keeps those at or below it, and at most
    max_events per pair are stored, the earliest.  pairs and both sides exactly as screen_pairs takes them.  The closest event of
    a pair carries, bit for bit, screen_pairs' distance and time for it; (i, j) and (j, i) give the same events.  An empty list
    returns an empty result without a library call.  devices=[d0, d1, ...]: contiguous blocks of the list's rows on several
    devices (every device holds both sides), written in place, the bits of one device."""
    pairs, src, cat, M, T0, T1, given_traj = _check_list_call("screen_events", pairs, T0, T1, eph, cat_eph, Y, units, span, ns, cat_Y, cat_units,
                                                              cat_span, cat_ns, M)
    if int(max_events) != max_events or max_events < 1:
        raise ValueError(f"max_events: need an integer >= 1, got {max_events}")
    thr = 0.0 if threshold is None else float(threshold)
    if not thr == thr:
        raise ValueError("threshold is NaN")
    n, E = pairs.shape[0], int(max_events)
    out = dict(events=np.empty((n, E, 4)), info=np.empty((n, E, 2), dtype=np.int32), count=np.zeros(n, dtype=np.int32),
               status=np.zeros(n, dtype=np.int32))
    statuses = _screen_list(pairs, out, device, devices, src=src, cat=cat, M=M, T0=T0, T1=T1, events=(thr, E))
    return EncounterEvents(out["events"], out["info"], out["count"], out["status"], *statuses)


def _check_max_shift(max_shift):
    """max_shift as the library takes it: None -> 0.0 (unlimited)"""
    if max_shift is None:
        return 0.0
    if not (np.ndim(max_shift) == 0 and max_shift == max_shift):
        raise ValueError(f"max_shift: need a number of seconds that is not NaN (None or <= 0: unlimited), got {max_shift}")
    return float(max_shift)


def screen_track(pairs, T0, T1, max_shift=None, eph=None, cat_eph=None, device=0, devices=None, *, Y=None, units=None, span=None, ns=None,
                 cat_Y=None, cat_units=None, cat_span=None, cat_ns=None, M=None):
    """The close approach of every LISTED row that lies nearest the row's own time, on the common grid linspace(T0, T1, M): an
    encounter followed through a re-screen.  screen_pairs returns a pair's global minimum, so after a manoeuvre two rows of the same
    pair (screen_events lists one per encounter) both read the same encounter; here each row (i, j, ., t_row) gets, of the pair's
    events as screen_events defines them WITHOUT a threshold, the one that minimises (|t - t_row|, grid interval).  pairs: (n, 4)
    rows, a ConjunctionResult or an EncounterEvents (its .events); columns 0, 1 and 3 are read.  Both sides exactly as screen_pairs
    takes them.  max_shift (seconds; None or <= 0: unlimited): only events with |t - t_row| <= max_shift count.  Returns (out, info,
    status): out (n, 4) rows (i, j, distance, time) in list order, info (n, 2) int32 (grid interval, 1 for an edge event else 0),
    status (n,) int32.  A row without an event, or with none inside max_shift, is (+inf, NaN), info (-1, 0), status 0; an index
    outside its side, i == j without a catalogue, or a t_row that is NaN or infinite is (NaN, NaN), (-1, 0), MPCX_ST_BADK = 9.  A
    finite t_row outside [T0, T1] picks the first or the last event.  From trajectories it returns (out, info, status, eph_status,
    cat_status).  A row of screen_events' or screen_pairs' output, given back on the same inputs, returns its own distance, time,
    interval and edge bit for bit.  An empty list returns empty arrays without a library call.  devices=[d0, d1, ...]: contiguous
    blocks of the list's rows on several devices (every device holds both sides), written in place, the bits of one device."""
    pairs, src, cat, M, T0, T1, given_traj = _check_list_call("screen_track", pairs, T0, T1, eph, cat_eph, Y, units, span, ns, cat_Y, cat_units,
                                                              cat_span, cat_ns, M)
    shift = _check_max_shift(max_shift)
    n = pairs.shape[0]
    out = dict(out=np.empty((n, 4)), info=np.empty((n, 2), dtype=np.int32), status=np.zeros(n, dtype=np.int32))
    statuses = _screen_list(pairs, out, device, devices, src=src, cat=cat, M=M, T0=T0, T1=T1, track=shift)
    return (out["out"], out["info"], out["status"], *statuses) if given_traj else (out["out"], out["info"], out["status"])


def cumulative_probability(events, pc):
    """The probability of at least one collision per list row of `events` (EncounterEvents): 1 - prod (1 - pc_e) over the row's
    events, taken as -expm1(sum log1p(-pc_e)) so that many small probabilities add up without cancellation.  pc (n_ev,): the
    events' probabilities, row for row of events.events (collision_probability(events.events, ...).pc, or that CollisionResult; a
    WindowCollisionResult of collision_probability_window over the same rows gives its p, one window per event).
    A row with an event whose pc is NaN is NaN; a row without events is 0.  The encounters are taken as independent."""
    pc = np.asarray(pc.pc if isinstance(pc, CollisionResult) else pc.p if isinstance(pc, WindowCollisionResult) else pc, dtype=np.float64)
    if pc.shape != events.row.shape:
        raise ValueError(f"pc: expected ({len(events.row)},) probabilities, one per stored event, got {pc.shape}")
    total = np.zeros(len(events.count))
    with np.errstate(divide="ignore", invalid="ignore"):
        np.add.at(total, events.row, np.log1p(-pc))
        return 0.0 - np.expm1(total)


def catalogue_trajectories(position_m, velocity_m_s, T0, T1, n, include_J2=True, device=0, devices=None):
    """A catalogue given as D state vectors at the epoch T0 (position_m (D, 3) metres, velocity_m_s (D, 3) m/s) -> (Y, units, span)
    for screen_against: every object propagated from T0 to T1 (seconds) in its own SatelliteScale units -- length = its radius at
    T0, time = the period of the circular orbit of that radius -- by propagate_batch with zero thrust and no drag, sampled at n
    uniform nodes.  Y (D, 7, n) normalised (the mass row is 1), units (D, 2) = (radius at T0, that period), span (D, 2) = (T0, T1)."""
    from .satellite_scale import SatelliteScale
    from .simulator import propagate_batch
    p, v = _ffi.as_f64(position_m), _ffi.as_f64(velocity_m_s)
    if p.ndim != 2 or p.shape[1] != 3 or p.shape[0] < 1 or v.shape != p.shape:
        raise ValueError(f"position_m, velocity_m_s: expected (D, 3) and (D, 3), got {p.shape} and {v.shape}")
    if not (np.isfinite(T0) and np.isfinite(T1) and T1 > T0):
        raise ValueError(f"need finite T0 < T1, got [{T0}, {T1}]")
    if int(n) != n or n < 2:
        raise ValueError(f"n: need an integer >= 2 nodes, got {n}")
    if not (np.isfinite(p).all() and np.isfinite(v).all() and (p != 0.0).any(axis=1).all()):
        raise ValueError("position_m, velocity_m_s: need finite states away from the origin")
    D = p.shape[0]
    state = np.column_stack([p, v, np.ones(D)])                      # unit mass: nothing here depends on it (no thrust, no drag)
    scales = [SatelliteScale(x=x) for x in state]
    units = np.array([[sc.units["length"], sc.units["time"]] for sc in scales], dtype=np.float64)
    y0 = np.stack([sc.normalize_state(x) for sc, x in zip(scales, state)])
    consts = np.stack([sc.get_normalized_constants().as_vector() for sc in scales])
    y, status, _ = propagate_batch(y0, (float(T1) - float(T0)) / units[:, 1], consts, (_ffi.CTRL_ZERO, None, 0, 1.0), int(n),
                                   include_drag=False, include_J2=include_J2, device=device, devices=devices)
    if (status != 0).any():
        raise RuntimeError(f"catalogue_trajectories: propagation failed: {[_ffi.STATUS_TEXT.get(int(c), c) for c in status if c]}")
    return y, units, np.tile([float(T0), float(T1)], (D, 1))


def combine(results):
    """Several screens of the same satellites over consecutive time windows (the flown segments) as one: per row the smallest
    distance, of equal ones the smaller partner, then the earlier window; per pair its smallest distance, the earlier window on a
    tie.  n_pairs_total counts the pairs of the union of the lists (exact when no window's list was cut off at max_pairs).
    status and cat_status are None: an ephemeris status belongs to one window's trajectories, so read it from the window's own
    result (ConstellationMPC.screen and screen_against with what="flown" combine their windows and therefore return neither)."""
    results = list(results)
    if not results:
        raise ValueError("combine: nothing to combine")
    dmin, partner, tca = results[0].dmin.copy(), results[0].partner.copy(), results[0].tca.copy()
    for r in results[1:]:
        none = partner < 0
        jr = np.where(r.partner < 0, np.iinfo(np.int32).max, r.partner)
        jb = np.where(none, np.iinfo(np.int32).max, partner)
        better = (r.partner >= 0) & (none | (r.dmin < dmin) | ((r.dmin == dmin) & (jr < jb)))
        dmin[better], partner[better], tca[better] = r.dmin[better], r.partner[better], r.tca[better]
    best = {}
    for r in results:
        for i, j, d, t in r.pairs:
            key = (int(i), int(j))
            if key not in best or d < best[key][0]:
                best[key] = (d, t)
    pairs = sort_pairs([(i, j, d, t) for (i, j), (d, t) in best.items()])
    total = max([len(pairs)] + [r.n_pairs_total for r in results])
    return ConjunctionResult(dmin, partner, tca, pairs, total)


# ---- from a pairs list to collision probabilities (include/mpcx.h: mpcx_covariance_batch, mpcx_collision_probability; csrc/collision.hip)
DEFAULT_MAX_STEP = Discretizer(None).ivp_max_step                        # the linearisation's step limit: whatever the Discretizer starts with


class CollisionResult:
    """For the n rows of `pairs` (i, j, distance, time), row for row: pc (n,) the collision probability, miss (n,) the miss distance
    in the encounter plane (m), speed (n,) the relative speed (m/s), sigma (n, 2) the combined position uncertainty along the
    principal axes of the encounter plane (m, larger first), mahalanobis (n,) the miss in units of it, status (n,) int32 MPCX_ST_*
    (a row whose status is not 0 is NaN in all of them)."""

    def __init__(self, pairs, out, status):
        self.pairs, self.status = pairs, status
        self.pc, self.miss, self.speed = out[:, _ffi.PC_P], out[:, _ffi.PC_MISS], out[:, _ffi.PC_SPEED]
        self.sigma, self.mahalanobis = out[:, _ffi.PC_SIGMA1:_ffi.PC_SIGMA2 + 1], out[:, _ffi.PC_MAHAL]

    def __repr__(self):
        return f"CollisionResult(pairs={len(self.pairs)})"


def _check_p0(P0, S, name="P0"):
    P0 = _ffi.as_f64(P0)
    if P0.shape == (6, 6):
        P0 = np.broadcast_to(P0, (S, 6, 6))
    if P0.shape != (S, 6, 6):
        raise ValueError(f"{name}: expected (6, 6) or ({S}, 6, 6) covariances of position (m) and velocity (m/s), got {P0.shape}")
    return _ffi.as_f64(P0)


def _check_q(q, S):
    if q is None:
        return None
    q = _per_row(q, S, "q", "acceleration noise densities (m^2/s^3)")
    if not (q >= 0.0).all():
        raise ValueError("q: need densities >= 0")
    return q


def _check_plan(Y, U, units, span, consts, ns, P=None, few="need", thrust_optional=False):
    """the plan a linearising call takes: trajectories of at least 2 nodes, the thrust at the nodes (None only where thrust_optional),
    the constants, and the covariances at the nodes where there are any -> (Y, U, units, span, consts, ns, P)"""
    Y, units, span, ns = _check_trajectories(Y, units, span, ns)
    S, _, K = Y.shape
    if K < 2:
        raise ValueError(f"Y: {few} at least 2 nodes, got {Y.shape}")
    if U is not None or not thrust_optional:
        U = _ffi.as_f64(U)
        if U.shape != (S, 3, K):
            raise ValueError(f"U: expected ({S}, 3, {K}) thrust at the nodes, got {U.shape}")
    consts = _ffi.as_f64(consts)
    if consts.shape != (S, _ffi.NCONST):
        raise ValueError(f"consts: expected ({S}, {_ffi.NCONST}) normalised constants per satellite, got {consts.shape}")
    if P is not None:
        P = _ffi.as_f64(P)
        if P.shape != (S, K, 6, 6):
            raise ValueError(f"P: expected ({S}, {K}, 6, 6) covariances at the nodes (covariance), got {P.shape}")
    return Y, U, units, span, consts, ns, P


def _covariance_problem(Y, units, span, consts, P0, U, ns, q):
    """what covariance and covariance_thrust share: the checks -> the batched inputs [Y, units, span, consts, P0, U, ns, q] and the
    result arrays P and status"""
    Y, U, units, span, consts, ns, _ = _check_plan(Y, U, units, span, consts, ns, few="a covariance needs", thrust_optional=True)
    S, _, n = Y.shape
    out = dict(P=_ffi.result_pool.take((S, n, 6, 6)), status=np.zeros(S, dtype=np.int32))
    return [Y, units, span, consts, _check_p0(P0, S), U, ns, _check_q(q, S)], out


def covariance(Y, units, span, consts, P0, U=None, ns=None, q=None, include_drag=False, include_J2=False, atmosphere=None,
               max_step=DEFAULT_MAX_STEP, device=0, devices=None, return_status=False):
    """The covariance of position (m) and velocity (m/s) at every node of S trajectories -> P (S, n, 6, 6).  Y (S, 7, n), units, span
    [, ns] as common_clock takes them; consts (S, 8) each satellite's normalised constants; P0 (6, 6) or (S, 6, 6) the covariance at
    the first node (its upper triangle is read); U (S, 3, n) the thrust at the nodes (None: zero thrust); q a scalar or (S,) white
    acceleration noise in m^2/s^3.  The device linearises about (Y, U, span) under the model include_drag / include_J2 / atmosphere
    (the Discretizer's) and chains the state-transition matrices of the node intervals: P_k+1 = Phi_k P_k Phi_k^T + q Q(h).
    A satellite with a node count outside 2..n, an empty span or a time unit that is not positive and finite, a failed linearisation
    or a non-finite P0 is NaN throughout
    (return_status=True returns (P, status) with its MPCX_ST_* code); nodes past ns come back zero.  devices=[d0, d1, ...]: contiguous
    blocks of satellites on several devices (sharding.sharded_call), written in place, the bits of one device."""
    batched, out = _covariance_problem(Y, units, span, consts, P0, U, ns, q)
    dispatch(_covariance_call, batched, out, device, devices, **_model(include_drag, include_J2, atmosphere, max_step))
    return (out["P"], out["status"]) if return_status else out["P"]


def _covariance_call(Y, units, span, consts, P0, U, ns, q, *, device, slot, out, flags, max_step, atmosphere):
    """one block of satellites on context (device, slot), P and status into `out` (the block's views)"""
    S, _, n = Y.shape
    _ffi.call("mpcx_covariance_batch", _context(device, slot, flags, atmosphere), S, n, _ffi.iptr_opt(ns), _ffi.dptr(Y), _ffi.dptr_opt(U),
              _ffi.dptr(units), _ffi.dptr(span), _ffi.dptr(consts), flags, max_step, _ffi.dptr(P0), _ffi.dptr_opt(q), _ffi.dptr(out["P"]),
              _ffi.iptr(out["status"]))


def gates_execution(scales, fixed_magnitude_N=0.0, proportional_magnitude=0.0, fixed_pointing_N=0.0, proportional_pointing_rad=0.0, off_N=0.0):
    """A Gates execution-error model given in physical units -- the fixed magnitude and pointing errors and the thrust below which the
    engine counts as off in newtons, the proportional magnitude error as a fraction, the proportional pointing error in radians per
    transverse axis; scalars or one value per satellite -- as covariance_thrust's execution (S, 5) = (s_fm, s_pm, s_fp, s_pp, u_off)
    in EACH satellite's own thrust unit (SatelliteScale.units["force"]): the counterpart of constellation_mpc.normalised_limits."""
    S = len(scales)
    force = np.array([sc.units["force"] for sc in scales], dtype=np.float64)
    per_sat = lambda v, name: _per_row(v, S, name, "values")
    out = np.column_stack([per_sat(fixed_magnitude_N, "fixed_magnitude_N") / force, per_sat(proportional_magnitude, "proportional_magnitude"),
                           per_sat(fixed_pointing_N, "fixed_pointing_N") / force, per_sat(proportional_pointing_rad, "proportional_pointing_rad"),
                           per_sat(off_N, "off_N") / force])
    if not (np.isfinite(out).all() and (out >= 0.0).all()):
        raise ValueError("gates_execution: need finite figures >= 0")
    return _ffi.as_f64(out)


def _check_execution(execution, S):
    execution = _ffi.as_f64(execution)
    if execution.shape == (_ffi.NEXEC,):
        execution = np.broadcast_to(execution, (S, _ffi.NEXEC))
    if execution.shape != (S, _ffi.NEXEC):
        raise ValueError(f"execution: expected ({_ffi.NEXEC},) or ({S}, {_ffi.NEXEC}) rows (s_fm, s_pm, s_fp, s_pp, u_off) "
                         f"(gates_execution), got {execution.shape}")
    return _ffi.as_f64(execution)


def covariance_thrust(Y, units, span, consts, P0, U, execution, mass_var0=None, ns=None, q=None, include_drag=False, include_J2=False,
                      atmosphere=None, max_step=DEFAULT_MAX_STEP, device=0, devices=None, return_status=False, return_mass=False):
    """covariance with thrust execution errors -> P (S, n, 6, 6), what every consumer of covariance's P takes.  The arguments are
    covariance's, with U (S, 3, n) required, and execution (5,) or (S, 5) = (s_fm, s_pm, s_fp, s_pp, u_off) in each satellite's own
    thrust unit (gates_execution makes it from newtons): at every node the executed thrust is u_k + e_k, e_k independent between nodes
    with covariance s_par^2 along u_k and s_perp^2 across it, s_par^2 = s_fm^2 + (s_pm |u_k|)^2, s_perp^2 = s_fp^2 + (s_pp |u_k|)^2, and
    none where |u_k| <= u_off; mass_var0 a scalar or (S,) mass variance at the first node in the satellite's mass unit squared.  The
    device chains all seven states of the linearisation with both first-order-hold input blocks (include/mpcx.h,
    mpcx_covariance_thrust_batch).  A satellite whose execution row is zero and whose mass_var0 is 0 gets covariance's bits.
    A failed satellite -- covariance's failures, or a negative or non-finite execution entry or mass_var0 -- is NaN throughout
    (return_status=True appends status).  return_mass=True appends Pm (S, n, 7): the mass's covariances with position and velocity
    and its variance.  The results come as P[, Pm][, status].  devices=[d0, d1, ...]: contiguous blocks of satellites on several
    devices (sharding.sharded_call), the bits of one device."""
    if U is None:
        raise ValueError("U: covariance_thrust needs the thrust at the nodes (without thrust: covariance)")
    batched, out = _covariance_problem(Y, units, span, consts, P0, U, ns, q)
    S, _, n = batched[0].shape
    batched += [_check_execution(execution, S), None if mass_var0 is None else _per_row(mass_var0, S, "mass_var0", "values")]
    if return_mass:
        out["Pm"] = np.empty((S, n, 7))
    dispatch(_covariance_thrust_call, batched, out, device, devices, **_model(include_drag, include_J2, atmosphere, max_step))
    res = (out["P"],) + ((out["Pm"],) if return_mass else ()) + ((out["status"],) if return_status else ())
    return res[0] if len(res) == 1 else res


def _covariance_thrust_call(Y, units, span, consts, P0, U, ns, q, execution, mass_var0, *, device, slot, out, flags, max_step, atmosphere):
    """one block of satellites on context (device, slot), P, Pm and status into `out` (the block's views)"""
    S, _, n = Y.shape
    _ffi.call("mpcx_covariance_thrust_batch", _context(device, slot, flags, atmosphere), S, n, _ffi.iptr_opt(ns), _ffi.dptr(Y), _ffi.dptr(U),
              _ffi.dptr(units), _ffi.dptr(span), _ffi.dptr(consts), flags, max_step, _ffi.dptr(P0), _ffi.dptr_opt(q), _ffi.dptr(execution),
              _ffi.dptr_opt(mass_var0), _ffi.dptr(out["P"]), _ffi.dptr_opt(out.get("Pm")), _ffi.iptr(out["status"]))


def _check_density(density, S):
    density = _ffi.as_f64(density)
    if density.shape == (_ffi.NDENS,):
        density = np.broadcast_to(density, (S, _ffi.NDENS))
    if density.shape != (S, _ffi.NDENS):
        raise ValueError(f"density: expected ({_ffi.NDENS},) or ({S}, {_ffi.NDENS}) rows (sigma, tau in seconds; np.inf: a bias), got {density.shape}")
    return _ffi.as_f64(density)


def covariance_drag(Y, units, span, consts, P0, density, U=None, execution=None, mass_var0=None, ns=None, q=None, include_J2=False,
                    atmosphere=None, max_step=DEFAULT_MAX_STEP, device=0, devices=None, return_status=False, return_mass=False,
                    return_density=False):
    """covariance_thrust with an uncertain drag -> P (S, n, 6, 6), what every consumer of covariance's P takes.  The drag is always
    in the model (include_J2 and atmosphere as in covariance).  density (2,) or (S, 2) = (sigma, tau): the drag acceleration of a
    satellite is (1 + beta) a_D, beta -- the fractional error of density times ballistic coefficient -- a zero-mean first-order
    Gauss-Markov process with stationary deviation sigma and correlation time tau in seconds (np.inf: a constant bias), held over
    each node interval, independent of P0, of the thrust errors and of q.  U (S, 3, n) the thrust at the nodes (None: zero thrust),
    execution and mass_var0 as in covariance_thrust (None: no execution error, no mass variance).  The device chains the eight
    states (position, velocity, mass, beta) with the drag column of one linearisation (include/mpcx.h, mpcx_covariance_drag_batch).
    A satellite with sigma = 0 gets covariance_thrust's bits, and with a zero execution row and no mass variance covariance's.
    A failed satellite -- covariance_thrust's failures, or a negative or non-finite sigma, or a tau that is <= 0 or NaN -- is NaN
    throughout (return_status=True appends status).  return_mass=True appends Pm (S, n, 7); return_density=True appends Pb (S, n, 8):
    beta's covariances with position (m), velocity (m/s) and mass, and its variance.  The results come as P[, Pm][, Pb][, status].
    Density errors common to two objects of a pair are not modelled: adding two such P as independent overstates the pair's
    relative covariance (Pb is what a cross term would be formed from).  devices=[d0, d1, ...]: contiguous blocks of satellites on
    several devices (sharding.sharded_call), the bits of one device."""
    batched, out = _covariance_problem(Y, units, span, consts, P0, U, ns, q)
    S, _, n = batched[0].shape
    if batched[5] is None:
        batched[5] = np.zeros((S, 3, n))
    batched += [None if execution is None else _check_execution(execution, S),
                None if mass_var0 is None else _per_row(mass_var0, S, "mass_var0", "values"), _check_density(density, S)]
    if return_mass:
        out["Pm"] = np.empty((S, n, 7))
    if return_density:
        out["Pb"] = np.empty((S, n, 8))
    dispatch(_covariance_drag_call, batched, out, device, devices, **_model(True, include_J2, atmosphere, max_step))
    res = (out["P"],) + ((out["Pm"],) if return_mass else ()) + ((out["Pb"],) if return_density else ()) + ((out["status"],) if return_status else ())
    return res[0] if len(res) == 1 else res


def _covariance_drag_call(Y, units, span, consts, P0, U, ns, q, execution, mass_var0, density, *, device, slot, out, flags, max_step, atmosphere):
    """one block of satellites on context (device, slot), P, Pm, Pb and status into `out` (the block's views)"""
    S, _, n = Y.shape
    _ffi.call("mpcx_covariance_drag_batch", _context(device, slot, flags, atmosphere), S, n, _ffi.iptr_opt(ns), _ffi.dptr(Y), _ffi.dptr(U),
              _ffi.dptr(units), _ffi.dptr(span), _ffi.dptr(consts), flags, max_step, _ffi.dptr(P0), _ffi.dptr_opt(q), _ffi.dptr_opt(execution),
              _ffi.dptr_opt(mass_var0), _ffi.dptr(density), _ffi.dptr(out["P"]), _ffi.dptr_opt(out.get("Pm")), _ffi.dptr_opt(out.get("Pb")),
              _ffi.iptr(out["status"]))


def _check_side(Y, units, span, P, radius, ns, pre=""):
    """one side of collision_probability: trajectories, their covariances and hard-body radii"""
    Y, units, span, ns = _check_trajectories(Y, units, span, ns, pre)
    S, _, n = Y.shape
    if n < 2:
        raise ValueError(f"{pre}Y: need at least 2 nodes, got {Y.shape}")
    if P is None or radius is None:
        raise ValueError(f"{pre}P and {pre}radius are required with {pre}Y")
    P = _ffi.as_f64(P)
    if P.shape != (S, n, 6, 6):
        raise ValueError(f"{pre}P: expected ({S}, {n}, 6, 6) covariances at the nodes (covariance), got {P.shape}")
    return Y, units, span, P, _per_row(radius, S, pre + "radius", "hard-body radii in m"), ns


def _check_cat_radii(cat):
    """cat = (cat_Y, cat_units, cat_span, cat_P, cat_radius[, cat_ns]) of the probabilities -> _check_side's tuple; None stays None"""
    if cat is None:
        return None
    if len(cat) not in (5, 6):
        raise ValueError(f"cat: expected (cat_Y, cat_units, cat_span, cat_P, cat_radius[, cat_ns]), got {len(cat)} items")
    return _check_side(*cat[:5], cat[5] if len(cat) == 6 else None, "cat_")


def _check_window(half_window, panels, n):
    """the window of every row of a list of n -> (half (n,), panels)"""
    half = _per_row(half_window, n, "half_window", "seconds")
    if np.ndim(panels) != 0 or int(panels) != panels or not 1 <= panels <= _ffi.PW_MAX_PANELS:
        raise ValueError(f"panels: need an integer in 1 .. {_ffi.PW_MAX_PANELS}, got {panels}")
    return half, int(panels)


def collision_probability(pairs, radius, Y, units, span, P, ns=None, cat=None, mu=None, device=0, devices=None):
    """The short-encounter collision probability of every listed pair -> CollisionResult.  pairs: (n, 4) rows (i, j, distance,
    time in s) as screen and screen_against list them, or their ConjunctionResult; radius a scalar or (S,) hard-body radii (m);
    Y, units, span [, ns] the trajectories that were screened and P (S, n, 6, 6) their covariances (covariance).  cat = (cat_Y,
    cat_units, cat_span, cat_P, cat_radius[, cat_ns]): j indexes this catalogue (screen_against's lists); None: j indexes the
    constellation (screen's).  mu: m^3/s^2, the constants' Earth value by default.  Each object's state and position covariance at
    the pair's time come from its own nodes (cubic Hermite; the covariance of the nearest node carried over the rest of the way by
    the two-body short-arc transition); the probability is the combined Gaussian's integral over the disc of the summed radii in
    the plane across the relative velocity, by a fixed 64-point rule: accurate to 1e-13 relative for radius / sigma <= 2, 2e-6 at 8,
    6e-3 at 20 (include/mpcx.h).  An empty list returns empty arrays without a library call.  devices=[d0, d1, ...]: contiguous
    blocks of the list's rows on several devices (every device holds all trajectories), written in place, the bits of one device."""
    pairs = _as_pairs(pairs)
    how = dict(rows=_check_side(Y, units, span, P, radius, ns), cols=_check_cat_radii(cat), mu=_check_mu(mu))
    n = pairs.shape[0]
    out = dict(out=np.empty((n, _ffi.NPC)), status=np.zeros(n, dtype=np.int32))
    if n:
        dispatch(_collision_call, [pairs], out, device, devices, **how)
    return CollisionResult(pairs, out["out"], out["status"])


def _collision_call(pairs, *, device, slot, out, rows, cols, mu):
    """one block of the list's rows on context (device, slot), into `out` (the block's views)"""
    pairs = _ffi.as_f64(pairs)
    _ffi.call("mpcx_collision_probability", _context(device, slot), len(pairs), _ffi.dptr(pairs), *_side_args(rows, 2), *_side_args(cols, 2), mu,
              _ffi.dptr(out["out"]), _ffi.iptr(out["status"]))


# ---- the same list over a time window (include/mpcx.h: mpcx_collision_probability_window; csrc/collision_window.hip)
DEFAULT_PANELS = 4


class WindowCollisionResult:
    """For the n rows of `pairs` (i, j, distance, time), row for row: p (n,) = min(1, start + entries), start (n,) the probability
    of being within the summed radii at the window's start, entries (n,) the expected number of entries into that sphere during
    the window, rate_max (n,) the largest entry rate at a time node (1/s) and t_rate_max (n,) its time (s), window (n, 2) the window
    used (the requested one cut to both objects' spans), status (n,) int32 MPCX_ST_* (a row whose status is not 0 is NaN in all of
    them)."""

    def __init__(self, pairs, out, status):
        self.pairs, self.status = pairs, status
        self.p, self.start, self.entries = out[:, _ffi.PW_P], out[:, _ffi.PW_START], out[:, _ffi.PW_ENTRIES]
        self.rate_max, self.t_rate_max, self.window = out[:, _ffi.PW_RATE_MAX], out[:, _ffi.PW_T_RATE_MAX], out[:, _ffi.PW_TA:_ffi.PW_TB + 1]

    def __repr__(self):
        return f"WindowCollisionResult(pairs={len(self.pairs)})"


def encounter_half_window(col, radius_sum, nsigma=8):
    """(nsigma sigma_1 + R) / speed per row of a CollisionResult, in seconds: the half window about the closest approach outside
    which the short-encounter model puts no probability -- the window inside which collision_probability_window and
    collision_probability must agree where the latter holds.  radius_sum: a scalar or (n,) summed hard-body radii R (m).  inf
    where the speed is 0 or NaN (a failed row, an encounter without relative motion): the caller chooses a window there."""
    if not isinstance(col, CollisionResult):
        raise ValueError(f"col: expected a CollisionResult, got {type(col).__name__}")
    n = len(col.speed)
    R = _per_row(radius_sum, n, "radius_sum", "summed radii in m")
    if not (np.ndim(nsigma) == 0 and nsigma > 0.0):
        raise ValueError(f"nsigma: need a number > 0, got {nsigma}")
    speed = np.asarray(col.speed, dtype=np.float64)
    moving = speed > 0.0                                                 # (False for NaN)
    h = np.full(n, np.inf)
    h[moving] = (float(nsigma) * np.asarray(col.sigma, dtype=np.float64)[moving, 0] + R[moving]) / speed[moving]
    return h


def collision_probability_window(pairs, radius, Y, units, span, P, half_window, panels=DEFAULT_PANELS, ns=None, cat=None, mu=None,
                                 device=0, devices=None):
    """The collision probability of every listed row over the time window [t - half_window, t + half_window] about the row's time
    -> WindowCollisionResult.  For encounters the short-encounter model of collision_probability does not cover: relative speeds of
    cm/s to m/s over minutes to a revolution, down to no relative motion at all.  pairs: (n, 4) rows (i, j, distance, time in s), a
    ConjunctionResult or an EncounterEvents (its .events: one window per event); radius, Y, units, span, P [, ns], cat and mu exactly
    as collision_probability takes them; half_window a scalar or (n,) of seconds (encounter_half_window for rows that have a
    relative speed); panels: the window is cut into that many equal panels of 64 time nodes (1 .. 64).  At every time node both
    objects' states come from their own nodes and their full 6 x 6 covariances are carried over from the nearest node; the result
    is the probability of being within the summed radii at the window's start plus the expected number of entries into that sphere
    during the window (a sphere integral of 512 points per time node): the probability of a collision in the window when no path
    enters twice, an upper bound otherwise (include/mpcx.h).  The window is cut to both objects' spans; a half window that is not
    positive and finite, or an empty cut window, is status 9 for that row.  An empty list returns empty arrays without a library call.
    devices=[d0, d1, ...]: contiguous blocks of the list's rows on several devices (every device holds all trajectories), written in
    place, the bits of one device."""
    pairs = _as_pairs(pairs)
    how = dict(rows=_check_side(Y, units, span, P, radius, ns), cols=_check_cat_radii(cat), mu=_check_mu(mu))
    n = pairs.shape[0]
    half, how["panels"] = _check_window(half_window, panels, n)
    out = dict(out=np.empty((n, _ffi.NPW)), status=np.zeros(n, dtype=np.int32))
    if n:
        dispatch(_collision_window_call, [pairs, half], out, device, devices, **how)
    return WindowCollisionResult(pairs, out["out"], out["status"])


def _collision_window_call(pairs, half, *, device, slot, out, rows, cols, mu, panels):
    """one block of the list's rows on context (device, slot), into `out` (the block's views)"""
    pairs, half = _ffi.as_f64(pairs), _ffi.as_f64(half)
    _ffi.call("mpcx_collision_probability_window", _context(device, slot), len(pairs), _ffi.dptr(pairs), *_side_args(rows, 2), *_side_args(cols, 2),
              mu, _ffi.dptr(half), panels, _ffi.dptr(out["out"]), _ffi.iptr(out["status"]))


# ---- the window of every listed row, chosen on the device (include/mpcx.h: mpcx_encounter_window; csrc/encounter_window.hip)
DEFAULT_NSIGMA, DEFAULT_LEVELS = 8, 3


class EncounterWindowResult:
    """For the n rows of `pairs` (i, j, distance, time), row for row: half (n,) seconds, what every half_window argument takes (the
    larger of the two reaches); window (n, 2) = (t - reach before, t + reach after) cut to both objects' spans; reach (n, 2) the
    first offsets before and after t known not to be live; g0 (n,) = g(t); flags (n,) int32 (1 clear, 2 open before, 4 open after, 8 a
    scan time was numerically bad and counted as live) with clear (n,) bool and open (n, 2) bool read from them; status (n,) int32
    MPCX_ST_* (a row whose status is not 0 is NaN in every column with flags 0)."""

    def __init__(self, pairs, out, flags, status):
        self.pairs, self.flags, self.status = pairs, flags, status
        self.half, self.window, self.g0 = out[:, _ffi.EW_HALF], out[:, _ffi.EW_TA:_ffi.EW_TB + 1], out[:, _ffi.EW_G0]
        self.reach = out[:, _ffi.EW_REACH_BEFORE:_ffi.EW_REACH_AFTER + 1]
        self.clear = (flags & _ffi.EW_CLEAR) != 0
        self.open = np.column_stack([(flags & _ffi.EW_OPEN_BEFORE) != 0, (flags & _ffi.EW_OPEN_AFTER) != 0])

    def __repr__(self):
        return f"EncounterWindowResult(pairs={len(self.pairs)}, clear={int(self.clear.sum())}, open={int(self.open.any(axis=1).sum())})"


def _check_search(max_half, nsigma, levels, n):
    """the search of every row of a list of n -> (max_half (n,), nsigma, levels)"""
    max_half = _per_row(max_half, n, "max_half", "seconds")
    if np.ndim(nsigma) != 0 or isinstance(nsigma, str) or not (nsigma > 0.0 and np.isfinite(nsigma)):
        raise ValueError(f"nsigma: need a positive finite number, got {nsigma}")
    if np.ndim(levels) != 0 or isinstance(levels, str) or int(levels) != levels or not 1 <= levels <= _ffi.EW_MAX_LEVELS:
        raise ValueError(f"levels: need an integer in 1 .. {_ffi.EW_MAX_LEVELS}, got {levels}")
    return max_half, float(nsigma), int(levels)


def encounter_window(pairs, radius, Y, units, span, P, max_half, nsigma=DEFAULT_NSIGMA, levels=DEFAULT_LEVELS, ns=None, cat=None, mu=None,
                     device=0, devices=None):
    """The time window about every listed row's own time outside which the pair's mean separation is more than nsigma combined
    sigmas, plus the summed radii, away from a collision -> EncounterWindowResult, whose .half is what collision_probability_window,
    collision_window_sensitivity, avoidance_window, avoidance_window_refine and collision_probability_mc take as half_window.  One
    rule for a crossing at km/s (a fraction of a second) and for a pair without relative motion (minutes, or all of max_half), where
    encounter_half_window has no answer.  pairs: (n, 4) rows (i, j, distance, time in s), a ConjunctionResult or an EncounterEvents;
    radius, Y, units, span, P [, ns], cat and mu exactly as collision_probability_window takes them; max_half a scalar or (n,) of
    seconds: how far from the row's time the search may go -- for the events of one pair, at most the spacing to the neighbouring
    event, since only the connected stretch about the row's time counts.  A time tau is live when |L^-1 d| - max(R, 0) |L^-1|_F -
    nsigma <= 0, with the mean relative position d and the Cholesky factor L of the combined position covariance at tau as
    collision_probability_window forms them; the Frobenius norm makes the rule conservative (include/mpcx.h).  Each side of the row's
    time is searched by `levels` (1 .. 4) refinements of 64 cells: a reach errs wide by at most max_half / 64^levels.  A side that
    is live all the way to max_half is open (its reach is max_half); a row whose own time is not live is clear and gets the smallest
    window, max_half / 64^levels.  A max_half that is not positive and finite is status 9 for that row.  An empty list returns empty
    arrays without a library call.  devices=[d0, d1, ...]: contiguous blocks of the list's rows on several devices (every device
    holds all trajectories), written in place, the bits of one device."""
    pairs = _as_pairs(pairs)
    how = dict(rows=_check_side(Y, units, span, P, radius, ns), cols=_check_cat_radii(cat), mu=_check_mu(mu))
    n = pairs.shape[0]
    max_half, how["nsigma"], how["levels"] = _check_search(max_half, nsigma, levels, n)
    out = dict(out=np.empty((n, _ffi.NEW)), flags=np.zeros(n, dtype=np.int32), status=np.zeros(n, dtype=np.int32))
    if n:
        dispatch(_encounter_window_call, [pairs, max_half], out, device, devices, **how)
    return EncounterWindowResult(pairs, out["out"], out["flags"], out["status"])


def _encounter_window_call(pairs, max_half, *, device, slot, out, rows, cols, mu, nsigma, levels):
    """one block of the list's rows on context (device, slot), into `out` (the block's views)"""
    pairs, max_half = _ffi.as_f64(pairs), _ffi.as_f64(max_half)
    _ffi.call("mpcx_encounter_window", _context(device, slot), len(pairs), _ffi.dptr(pairs), *_side_args(rows, 2), *_side_args(cols, 2), mu,
              _ffi.dptr(max_half), nsigma, levels, _ffi.dptr(out["out"]), _ffi.iptr(out["flags"]), _ffi.iptr(out["status"]))


# ---- the same list by sampled flights through the truth model (include/mpcx.h: mpcx_collision_probability_mc; csrc/collision_mc.hip)
DEFAULT_PROP_MAX_STEP = 1e-3                                             # the flights' step limit (avoidance_window_refine's)


class MonteCarloCollisionResult:
    """For the n rows of `pairs`, row for row, from N sampled worlds: p_hit (n,) the fraction of surviving samples in which the two
    flown objects came within the summed radii during the window, se_hit (n,) its binomial standard error; start, entries (n,) the
    sampled counterparts of the window rule's START and ENTRIES (the mean of inside_start, the mean number of entries), se_bound (n,)
    the standard error of the mean of inside_start + entries; excess (n,) = start + entries - p_hit, what the window rule's figure
    lies above the probability because paths re-enter; window (n, 2); n_ok (n,) the samples that survived their flights; counts (n, 6)
    int64 = (flown, failed, sum inside_start, sum entries, sum (inside_start + entries)^2, sum hit); status (n,) int32 MPCX_ST_* (a
    row whose status is not 0 is NaN in all but counts, which are 0).  With return_samples: samples (n, N, 5) = (dmin in m, t_min in
    s, inside_start, entries, flight status) per sample; with return_trajectories: Y_samples (n, NS, N, 7, K) and U_samples
    (n, NS, N, 3, K), the row side's flown trajectories and executed thrust tables (NS = 2: slots i, j; 1 with a catalogue)."""

    def __init__(self, pairs, out, counts, status, samples=None, Y_samples=None, U_samples=None):
        self.pairs, self.counts, self.status = pairs, counts, status
        self.p_hit, self.se_hit, self.start, self.entries = (out[:, c] for c in (_ffi.MC_P_HIT, _ffi.MC_SE_HIT, _ffi.MC_START, _ffi.MC_ENTRIES))
        self.se_bound, self.excess, self.n_ok = out[:, _ffi.MC_SE_BOUND], out[:, _ffi.MC_EXCESS], out[:, _ffi.MC_N_OK]
        self.window = out[:, _ffi.MC_TA:_ffi.MC_TB + 1]
        self.samples, self.Y_samples, self.U_samples = samples, Y_samples, U_samples

    def __repr__(self):
        return f"MonteCarloCollisionResult(pairs={len(self.pairs)}, samples={int(self.counts[:, _ffi.MCC_FLOWN].max(initial=0))})"

    def cumulative(self, events):
        """Per list row of `events` (EncounterEvents whose .events are this result's rows): the fraction of worlds with a hit in ANY of
        the row's events -> (p (n_rows,), se (n_rows,)).  Sample s is the same world in every row (the draws of an object do not
        depend on the row), so the per-sample records are joint samples; a world in which any of the row's events has a failed
        flight is left out.  cumulative_probability joins the same events as if they were independent.  A row without events is 0;
        a row with a failed event, or without a surviving world, is NaN.  Needs return_samples=True."""
        if self.samples is None:
            raise ValueError("cumulative: the per-sample records are needed (return_samples=True)")
        if len(events.row) != len(self.pairs):
            raise ValueError(f"cumulative: expected events with {len(self.pairs)} stored events, one per row of this result, got {len(events.row)}")
        rows = len(events.count)
        N = self.samples.shape[1]
        hit = (self.samples[:, :, _ffi.MS_INSIDE_START] + self.samples[:, :, _ffi.MS_ENTRIES]) >= 1.0
        good = self.samples[:, :, _ffi.MS_STATUS] == 0.0
        any_hit, all_good, failed = np.zeros((rows, N), dtype=bool), np.ones((rows, N), dtype=bool), np.zeros(rows, dtype=bool)
        for e, r in enumerate(np.asarray(events.row)):
            any_hit[r] |= hit[e]
            all_good[r] &= good[e]
            failed[r] |= self.status[e] != 0
        ok = all_good.sum(axis=1).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            p = (any_hit & all_good).sum(axis=1) / ok
            se = np.sqrt(p * (1.0 - p) / ok)
        p[failed], se[failed] = np.nan, np.nan
        none = np.asarray(events.count) == 0
        p[none], se[none] = 0.0, 0.0
        return p, se


def _check_mc_cat(cat):
    """cat = (cat_Y, cat_units, cat_span, cat_consts, cat_P0, cat_radius[, cat_ns]) of collision_probability_mc -> (Y, units, span, ns,
    consts, P0, radius); None stays None"""
    if cat is None:
        return None
    if len(cat) not in (6, 7):
        raise ValueError(f"cat: expected (cat_Y, cat_units, cat_span, cat_consts, cat_P0, cat_radius[, cat_ns]), got {len(cat)} items")
    Y, units, span, ns = _check_trajectories(cat[0], cat[1], cat[2], cat[6] if len(cat) == 7 else None, "cat_")
    D, _, K = Y.shape
    if K < 2:
        raise ValueError(f"cat_Y: need at least 2 nodes, got {Y.shape}")
    consts = _ffi.as_f64(cat[3])
    if consts.shape != (D, _ffi.NCONST):
        raise ValueError(f"cat_consts: expected ({D}, {_ffi.NCONST}) normalised constants per object, got {consts.shape}")
    return Y, units, span, ns, consts, _check_p0(cat[4], D, "cat_P0"), _per_row(cat[5], D, "cat_radius", "hard-body radii in m")


def _check_samples(samples, seed, scan, max_flights):
    for name, v, low in (("samples", samples, 1), ("scan", scan, 1), ("max_flights", max_flights, 0)):
        if np.ndim(v) != 0 or int(v) != v or not low <= v < 2 ** 31:
            raise ValueError(f"{name}: need an integer >= {low}, got {v}")
    if np.ndim(seed) != 0 or int(seed) != seed or not 0 <= seed < 2 ** 64:
        raise ValueError(f"seed: need an integer in 0 .. 2^64 - 1, got {seed}")
    return int(samples), int(seed), int(scan), int(max_flights)


def collision_probability_mc(pairs, radius, Y, U, units, span, consts, P0, half_window, samples, seed=0, scan=64, execution=None,
                             mass_var0=None, ns=None, cat=None, include_drag=False, include_J2=False, atmosphere=None,
                             prop_max_step=DEFAULT_PROP_MAX_STEP, max_flights=0, return_samples=False, return_trajectories=False, device=0,
                             devices=None):
    """The collision probability of every listed row over [t - half_window, t + half_window] by `samples` sampled flights through the
    nonlinear dynamics -> MonteCarloCollisionResult.  Nothing is linearised: in every sampled world each object starts from its first
    node plus a draw from P0 ((6, 6) or (S, 6, 6); m, m/s; positive semi-definite), its mass plus a draw of variance mass_var0, flies
    the plan's thrust U (S, 3, n; None: zero thrust) with the execution errors execution ((5,) or (S, 5), gates_execution; None:
    perfect execution) drawn at every node, under the model include_drag / include_J2 / atmosphere with the step limit prop_max_step;
    the window is scanned in `scan` intervals for the two flown objects coming within the summed radii (include/mpcx.h:
    mpcx_collision_probability_mc).  pairs, radius, Y, units, span, consts [, ns] and half_window as collision_probability_window and
    covariance take them.  cat = (cat_Y, cat_units, cat_span, cat_consts, cat_P0, cat_radius[, cat_ns]): j indexes this catalogue,
    whose objects fly without thrust.  The figure corresponds to covariance / covariance_thrust with q = 0 followed by
    collision_probability_window -- of which start + entries is the counterpart and p_hit what it bounds from above.
    The draws are Philox on (seed, sample, object): the same seed gives the same bits whatever the list, the devices or max_flights
    (0: the library's default; otherwise a bound on the trajectories in flight at once, hence on the workspace); a satellite in
    several rows flies the same trajectory in all of them.  An empty list returns empty arrays without a library call.
    devices=[d0, d1, ...]: contiguous blocks of the list's rows on several devices, the bits of one device."""
    pairs = _as_pairs(pairs)
    Y, U, units, span, consts, ns, _ = _check_plan(Y, U, units, span, consts, ns, thrust_optional=True)
    S, _, K = Y.shape
    cols = _check_mc_cat(cat)
    n, NS = pairs.shape[0], 1 if cols is not None else 2
    half, _ = _check_window(half_window, 1, n)
    N, seed, scan, max_flights = _check_samples(samples, seed, scan, max_flights)
    model = _model(include_drag, include_J2, atmosphere, prop_max_step)
    how = dict(rows=(Y, U, units, span, consts, ns, _check_p0(P0, S), None if execution is None else _check_execution(execution, S),
                     None if mass_var0 is None else _per_row(mass_var0, S, "mass_var0", "values"), _per_row(radius, S, "radius", "hard-body radii in m")),
               cols=cols, scan=scan, samples=N, seed=seed, max_flights=max_flights, flags=model["flags"], prop_max_step=model["max_step"],
               atmosphere=model["atmosphere"])
    out = dict(out=np.empty((n, _ffi.NMC)), counts=np.zeros((n, _ffi.NMCC), dtype=np.int64), status=np.zeros(n, dtype=np.int32),
               samples=np.empty((n, N, _ffi.NMS)) if return_samples else None,
               Y_samples=np.empty((n, NS, N, 7, K)) if return_trajectories else None,
               U_samples=np.empty((n, NS, N, 3, K)) if return_trajectories else None)
    if n:
        dispatch(_collision_mc_call, [pairs, half], out, device, devices, **how)
    return MonteCarloCollisionResult(pairs, out["out"], out["counts"], out["status"], out["samples"], out["Y_samples"], out["U_samples"])


def _collision_mc_call(pairs, half, *, device, slot, out, rows, cols, scan, samples, seed, max_flights, flags, prop_max_step, atmosphere):
    """one block of the list's rows on context (device, slot), into `out` (the block's views)"""
    Y, U, units, span, consts, ns, P0, execution, mass_var0, radius = rows
    pairs, half = _ffi.as_f64(pairs), _ffi.as_f64(half)
    if cols is None:
        cat = (0, 0) + (None,) * 7
    else:
        cY, cunits, cspan, cns, cconsts, cP0, cradius = cols
        cat = (cY.shape[0], cY.shape[2], _ffi.iptr_opt(cns), *[_ffi.dptr(a) for a in (cY, cunits, cspan, cconsts, cP0, cradius)])
    _ffi.call("mpcx_collision_probability_mc", _context(device, slot, flags, atmosphere), len(pairs), _ffi.dptr(pairs), Y.shape[0], Y.shape[2],
              _ffi.iptr_opt(ns), _ffi.dptr(Y), _ffi.dptr_opt(U), _ffi.dptr(units), _ffi.dptr(span), _ffi.dptr(consts), flags, prop_max_step,
              _ffi.dptr(P0), _ffi.dptr_opt(execution), _ffi.dptr_opt(mass_var0), _ffi.dptr(radius), *cat, _ffi.dptr(half), scan, samples, seed,
              max_flights, _ffi.lptr(out["counts"]), _ffi.dptr(out["out"]), _ffi.iptr(out["status"]),
              _ffi.dptr_opt(out.get("samples")), _ffi.dptr_opt(out.get("Y_samples")), _ffi.dptr_opt(out.get("U_samples")))


def catalogue_covariance(position_m, velocity_m_s, P0, T0, T1, n, q=None, include_J2=True, max_step=DEFAULT_MAX_STEP, device=0,
                         devices=None):
    """catalogue_trajectories followed by covariance -> (Y, units, span, P): a catalogue given as D state vectors at the epoch T0 with
    the covariance P0 ((6, 6) or (D, 6, 6); m, m/s) of each, propagated to T1 and sampled at n nodes, no thrust and no drag, every
    object linearised under its own SatelliteScale constants.  What collision_probability takes as cat, beside the radii."""
    from .satellite_scale import SatelliteScale
    Y, units, span = catalogue_trajectories(position_m, velocity_m_s, T0, T1, n, include_J2=include_J2, device=device, devices=devices)
    state = np.column_stack([_ffi.as_f64(position_m), _ffi.as_f64(velocity_m_s), np.ones(len(Y))])
    consts = np.stack([SatelliteScale(x=x).get_normalized_constants().as_vector() for x in state])
    P = covariance(Y, units, span, consts, P0, q=q, include_J2=include_J2, max_step=max_step, device=device, devices=devices)
    return Y, units, span, P


# ---- from a pairs list to avoidance manoeuvres (include/mpcx.h: mpcx_avoidance; csrc/avoidance.hip)
_WHO = {"i": 0, "j": 1, "both": 2}


class AvoidanceResult:
    """For the n rows of `pairs` (i, j, distance, time), row for row: d0 (n,) the distance now and d1 (n,) the predicted distance
    after the manoeuvre, both in the target's metric (metres, or Mahalanobis with covariances); dm (n, 2) the encounter-plane
    displacement in the (e_1, e_2) frame (m); miss1 (n,) the predicted miss |m + dm| (m); dt (n,) the shift of the time of closest
    approach (s); dv (n, 2) the cost per object, sum of w_m |da_m| (m/s), and umax (n, 2) its largest thrust change max_m |du_m|
    (normalised, to compare with u_max) -- column 0 object i, column 1 object j, 0 for one that does not move; du (n, NS, 3, K) the
    thrust change per node in the plan's own units (NS = 2: slots i, j; NS = 1 against a catalogue), sens (n, NS, 3, 3, K) the
    sensitivities g_m (row e_1 / e_2 / e_w, thrust component, node) or None; status (n,) int32 MPCX_ST_* (a row whose status is not
    0 is NaN in all of them)."""

    def __init__(self, pairs, out, du, sens, status):
        self.pairs, self.du, self.sens, self.status = pairs, du, sens, status
        self.d0, self.d1, self.miss1, self.dt = out[:, _ffi.AV_D0], out[:, _ffi.AV_D1], out[:, _ffi.AV_MISS1], out[:, _ffi.AV_DT]
        self.dm = out[:, _ffi.AV_DM1:_ffi.AV_DM2 + 1]
        self.dv, self.umax = out[:, _ffi.AV_DV_I:_ffi.AV_DV_J + 1], out[:, _ffi.AV_UMAX_I:_ffi.AV_UMAX_J + 1]
        self.out = out

    def __repr__(self):
        return f"AvoidanceResult(pairs={len(self.pairs)})"

    def apply(self, U, row):
        """a copy of the plan thrust U (S, 3, K) with pair `row`'s du added to its satellites"""
        U = np.array(U, dtype=np.float64)
        if U.ndim != 3 or U.shape[1:] != self.du.shape[2:]:
            raise ValueError(f"U: expected (S, 3, {self.du.shape[3]}) plan thrust, got {U.shape}")
        if self.status[row] != 0:
            raise ValueError(f"pair {row} has no manoeuvre: {_ffi.STATUS_TEXT.get(int(self.status[row]), int(self.status[row]))}")
        for slot in range(self.du.shape[1]):
            U[int(self.pairs[row, slot])] += self.du[row, slot]
        return U


def _check_who(who, against_catalogue=False):
    """who = 'i', 'j' or 'both' as the library takes it"""
    if who not in _WHO:
        raise ValueError(f"who: expected 'i', 'j' or 'both', got {who!r}")
    if against_catalogue and who != "i":
        raise ValueError(f"who = {who!r}: against a catalogue only the satellite can manoeuvre (who='i')")
    return _WHO[who]


def _check_cat(cat):
    """cat = (cat_Y, cat_units, cat_span[, cat_P][, cat_ns]) of avoidance -> (Y, units, span, ns, P or None)"""
    if not 3 <= len(cat) <= 5:
        raise ValueError(f"cat: expected (cat_Y, cat_units, cat_span[, cat_P][, cat_ns]), got {len(cat)} items")
    rest = list(cat[3:])
    P = rest.pop(0) if rest and rest[0] is not None and np.ndim(rest[0]) == 4 else None
    if len(rest) > 1:
        raise ValueError("cat: after cat_span come cat_P (D, n, 6, 6) and cat_ns (D,), in this order")
    Y, units, span, ns = _check_trajectories(cat[0], cat[1], cat[2], rest[0] if rest else None, "cat_")
    if Y.shape[2] < 2:
        raise ValueError(f"cat_Y: need at least 2 nodes, got {Y.shape}")
    if P is not None:
        P = _ffi.as_f64(P)
        if P.shape != (Y.shape[0], Y.shape[2], 6, 6):
            raise ValueError(f"cat_P: expected ({Y.shape[0]}, {Y.shape[2]}, 6, 6) covariances at the nodes (covariance), got {P.shape}")
    return Y, units, span, ns, P


def _encounter_problem(pairs, target, Y, U, units, span, consts, ns, P, cat, mu):
    """the checks every avoidance call makes of the list, the target, the plan, the covariances and the catalogue
    -> (pairs, Y, U, units, span, consts, ns, P, cols, mu)"""
    pairs = _as_pairs(pairs)
    if not (np.ndim(target) == 0 and np.isfinite(target) and target > 0.0):
        raise ValueError(f"target: need a positive finite distance, got {target}")
    plan = _check_plan(Y, U, units, span, consts, ns, P)
    cols = None if cat is None else _check_cat(cat)
    if cols is not None and (P is None) != (cols[4] is None):
        raise ValueError("P and cat_P come together (a Mahalanobis target) or not at all (a target in metres)")
    return (pairs, *plan, cols, _check_mu(mu))


def avoidance(pairs, target, Y, U, units, span, consts, ns=None, P=None, cat=None, who="i", include_drag=False, include_J2=False,
              atmosphere=None, max_step=DEFAULT_MAX_STEP, mu=None, return_sensitivities=False, device=0, devices=None):
    """The least-effort thrust change that opens every listed close approach to `target` -> AvoidanceResult.  pairs: (n, 4) rows
    (i, j, distance, time in s) as screen and screen_against list them, or their ConjunctionResult; Y (S, 7, n), U (S, 3, n), units,
    span, consts (S, 8) [, ns] the plan that was screened, linearised under include_drag / include_J2 / atmosphere as covariance
    does.  P (S, n, 6, 6) (covariance): target is a Mahalanobis distance in the combined encounter-plane covariance; None: target is
    a miss distance in metres.  cat = (cat_Y, cat_units, cat_span[, cat_P][, cat_ns]): j indexes this catalogue and only the
    satellite moves (cat_P exactly when P is given); None: j indexes the constellation and who = "i", "j" or "both" says which of the
    two moves.  The device sweeps the adjoint of the encounter-plane miss backwards over the linearisation's A, B_kn, B_kp to the
    derivative with respect to every thrust node (return_sensitivities=True returns them), and moves the miss in the direction that
    gains distance fastest per unit of effort -- the first-order optimum, not the optimum over the whole target ellipse
    (include/mpcx.h).  A pair already at or beyond the target gets du = 0.  An empty list returns empty arrays without a library
    call.  devices=[d0, d1, ...]: contiguous blocks of the list's rows on several devices, written in place, the bits of one device."""
    _check_who(who)
    pairs, Y, U, units, span, consts, ns, P, cols, mu = _encounter_problem(pairs, target, Y, U, units, span, consts, ns, P, cat, mu)
    n, K, NS = pairs.shape[0], Y.shape[2], 1 if cols is not None else 2
    out = dict(out=np.empty((n, _ffi.NAV)), du=_ffi.result_pool.take((n, NS, 3, K)),
               sens=_ffi.result_pool.take((n, NS, 3, 3, K)) if return_sensitivities else None, status=np.zeros(n, dtype=np.int32))
    how = dict(rows=(Y, U, units, span, consts, ns, P), cols=cols, mu=mu, target=float(target), who=_check_who(who, cols is not None),
               **_model(include_drag, include_J2, atmosphere, max_step))
    if n:
        dispatch(_avoidance_call, [pairs], out, device, devices, **how)
    return AvoidanceResult(pairs, out["out"], out["du"], out["sens"], out["status"])


def _plan_args(Y, U, units, span, consts, ns, flags, max_step):
    """the plan and the model of its linearisation as the library takes them, from S to max_step"""
    return (Y.shape[0], Y.shape[2], _ffi.iptr_opt(ns), _ffi.dptr(Y), _ffi.dptr(U), _ffi.dptr(units), _ffi.dptr(span), _ffi.dptr(consts), flags,
            max_step)


def _avoidance_call(pairs, *, device, slot, out, rows, cols, mu, target, who, flags, max_step, atmosphere):
    """one block of the list's rows on context (device, slot), into `out` (the block's views)"""
    Y, U, units, span, consts, ns, P = rows
    pairs = _ffi.as_f64(pairs)
    _ffi.call("mpcx_avoidance", _context(device, slot, flags, atmosphere), len(pairs), _ffi.dptr(pairs),
              *_plan_args(Y, U, units, span, consts, ns, flags, max_step), _ffi.dptr_opt(P), *_side_args(cols, 1), mu, target, who,
              _ffi.dptr(out["out"]), _ffi.dptr(out["du"]), _ffi.dptr_opt(out.get("sens")), _ffi.iptr(out["status"]))


# ---- avoidance for slow encounters (include/mpcx.h: mpcx_collision_window_sensitivity, mpcx_avoidance_window;
# csrc/collision_window.hip, csrc/avoidance_window.hip)
class WindowSensitivityResult(WindowCollisionResult):
    """WindowCollisionResult of the rows -- the bytes collision_probability_window returns -- and sens (n, NS, 3, K): the derivative of
    start + entries with respect to every thrust node (thrust component, node; the plan's normalised units) of the objects that move
    (NS = 2: slots i, j; NS = 1 against a catalogue; 0 for one that does not move), state_grad (n, 64 panels + 1, 6) the derivative
    with respect to the mean relative position and velocity at every time node, weighted, the ball term last, or None."""

    def __init__(self, pairs, out, sens, state_grad, status):
        super().__init__(pairs, out, status)
        self.sens, self.state_grad = sens, state_grad

    def __repr__(self):
        return f"WindowSensitivityResult(pairs={len(self.pairs)})"


class AvoidanceWindowResult:
    """For the n rows of `pairs` (i, j, distance, time), row for row: p0 (n,) the window figure start + entries now and p1 (n,) the
    same rule at the moved means, alpha (n,) the step, dq_linear (n,) the first-order prediction of p1 - p0, dv (n, 2) the cost per
    object, sum of w_m |da_m| (m/s), and umax (n, 2) its largest thrust change max_m |du_m| (normalised) -- column 0 object i, column
    1 object j, 0 for one that does not move --, evals (n,) the evaluations of the window rule made; du (n, NS, 3, K) the thrust
    change per node in the plan's own units (NS = 2: slots i, j; NS = 1 against a catalogue), sens (n, NS, 3, K) the derivative of
    start + entries with respect to the thrust nodes or None; status (n,) int32 MPCX_ST_* (a row whose status is not 0 is NaN in out
    and du)."""

    def __init__(self, pairs, out, du, sens, status):
        self.pairs, self.du, self.sens, self.status = pairs, du, sens, status
        self.p0, self.p1, self.alpha, self.dq_linear = out[:, _ffi.AW_P0], out[:, _ffi.AW_P1], out[:, _ffi.AW_ALPHA], out[:, _ffi.AW_DQ_LINEAR]
        self.dv, self.umax = out[:, _ffi.AW_DV_I:_ffi.AW_DV_J + 1], out[:, _ffi.AW_UMAX_I:_ffi.AW_UMAX_J + 1]
        self.evals = out[:, _ffi.AW_EVALS]
        self.out = out

    def __repr__(self):
        return f"AvoidanceWindowResult(pairs={len(self.pairs)})"

    apply = AvoidanceResult.apply


def _window_problem(pairs, radius, Y, U, units, span, consts, P, half_window, panels, ns, cat, who, mu):
    """the checks the window avoidance calls make: avoidance's of the list, the plan and who moves, and collision_probability_window's
    of the covariances, the radii, the catalogue, the half windows and the panels -> the keywords pairs and half and those of the
    block functions up to who"""
    _check_who(who)
    if P is None:
        raise ValueError("P: the covariances at the nodes (covariance) are required")
    pairs = _as_pairs(pairs)
    Y, U, units, span, consts, ns, P = _check_plan(Y, U, units, span, consts, ns, P)
    cols = _check_cat_radii(cat)
    half, panels = _check_window(half_window, panels, pairs.shape[0])
    rows = _check_side(Y, units, span, P, radius, ns) + (U, consts)
    return pairs, half, dict(rows=rows, cols=cols, mu=_check_mu(mu), panels=panels, who=_check_who(who, cols is not None))


def _window_arrays(n, how, return_sensitivities):
    """the result arrays both window manoeuvres share, for a list of n rows of the problem `how`"""
    K, NS = how["rows"][0].shape[2], 1 if how["cols"] is not None else 2
    return dict(out=np.empty((n, _ffi.NAW)), du=_ffi.result_pool.take((n, NS, 3, K)),
                sens=_ffi.result_pool.take((n, NS, 3, K)) if return_sensitivities else None, status=np.zeros(n, dtype=np.int32))


def _check_solve(target_p, tol, max_eval):
    """the step search of the window manoeuvres as the block functions take it: the keywords target_p, tol and max_eval"""
    if not (np.ndim(target_p) == 0 and 0.0 < target_p < 1.0):
        raise ValueError(f"target_p: need a probability strictly between 0 and 1, got {target_p}")
    if not (np.ndim(tol) == 0 and np.isfinite(tol) and tol > 0.0):
        raise ValueError(f"tol: need a positive finite number, got {tol}")
    if np.ndim(max_eval) != 0 or int(max_eval) != max_eval or max_eval < 1:
        raise ValueError(f"max_eval: need an integer >= 1, got {max_eval}")
    return dict(target_p=float(target_p), tol=float(tol), max_eval=int(max_eval))


def _check_rounds(rounds, prop_max_step):
    """the flights of the refine calls -> (rounds, prop_max_step)"""
    if not (np.ndim(rounds) == 0 and int(rounds) == rounds and rounds >= 0):
        raise ValueError(f"rounds: need an integer >= 0, got {rounds}")
    if not prop_max_step > 0.0:
        raise ValueError(f"prop_max_step: need > 0, got {prop_max_step}")
    return int(rounds), float(prop_max_step)


def collision_window_sensitivity(pairs, radius, Y, U, units, span, consts, P, half_window, panels=DEFAULT_PANELS, ns=None, cat=None,
                                 who="i", include_drag=False, include_J2=False, atmosphere=None, max_step=DEFAULT_MAX_STEP, mu=None,
                                 return_state_gradient=False, device=0, devices=None):
    """collision_probability_window together with the derivative of start + entries with respect to every thrust node of the objects
    that move -> WindowSensitivityResult.  pairs, radius, Y, units, span, P, half_window, panels [, ns], cat and mu exactly as
    collision_probability_window takes them (an EncounterEvents included); U (S, 3, n), consts (S, 8) and include_drag / include_J2 /
    atmosphere / max_step the plan and the model of its linearisation as avoidance takes them; who = "i", "j" or "both" says which
    object of a row moves (against a catalogue only "i").  The thrust moves the mean relative state only: the covariances, the window
    and the row's time are held (include/mpcx.h).  An empty list returns empty arrays without a library call.  devices=[d0, d1,
    ...]: contiguous blocks of the list's rows on several devices, written in place, the bits of one device."""
    pairs, half, how = _window_problem(pairs, radius, Y, U, units, span, consts, P, half_window, panels, ns, cat, who, mu)
    n, K, NS = pairs.shape[0], how["rows"][0].shape[2], 1 if how["cols"] is not None else 2
    out = dict(out=np.empty((n, _ffi.NPW)), sens=_ffi.result_pool.take((n, NS, 3, K)),
               state_grad=_ffi.result_pool.take((n, 64 * how["panels"] + 1, 6)) if return_state_gradient else None,
               status=np.zeros(n, dtype=np.int32))
    how.update(_model(include_drag, include_J2, atmosphere, max_step))
    if n:
        dispatch(_window_sensitivity_call, [pairs, half], out, device, devices, **how)
    return WindowSensitivityResult(pairs, out["out"], out["sens"], out["state_grad"], out["status"])


def _window_args(pairs, half, rows, cols, mu, panels, who, flags, max_step):
    """the arguments the window calls share, from n to who"""
    Y, units, span, P, radius, ns, U, consts = rows
    return (len(pairs), _ffi.dptr(pairs), *_plan_args(Y, U, units, span, consts, ns, flags, max_step), _ffi.dptr(P), _ffi.dptr(radius),
            *_side_args(cols, 2), mu, _ffi.dptr(half), panels, who)


def _window_sensitivity_call(pairs, half, *, device, slot, out, rows, cols, mu, panels, who, flags, max_step, atmosphere):
    """one block of the list's rows on context (device, slot), into `out` (the block's views)"""
    pairs, half = _ffi.as_f64(pairs), _ffi.as_f64(half)
    _ffi.call("mpcx_collision_window_sensitivity", _context(device, slot, flags, atmosphere),
              *_window_args(pairs, half, rows, cols, mu, panels, who, flags, max_step),
              _ffi.dptr(out["out"]), _ffi.dptr(out["sens"]), _ffi.dptr_opt(out.get("state_grad")), _ffi.iptr(out["status"]))


def avoidance_window(pairs, target_p, radius, Y, U, units, span, consts, P, half_window, panels=DEFAULT_PANELS, ns=None, cat=None,
                     who="i", tol=_ffi.AW_DEFAULT_TOL, max_eval=_ffi.AW_DEFAULT_MAX_EVAL, include_drag=False, include_J2=False,
                     atmosphere=None, max_step=DEFAULT_MAX_STEP, mu=None, return_sensitivities=False, device=0, devices=None):
    """The thrust change of least effort, to first order, that brings the window probability of every listed row down to target_p
    -> AvoidanceWindowResult.  For the rows collision_probability_window is for: pairs too slow for an encounter plane, which
    avoidance cannot aim at.  The arguments are collision_window_sensitivity's, with target_p strictly between 0 and 1, tol the
    tolerance on |ln(p1 / target_p)| and max_eval the most evaluations of the window rule a row may use.  The direction is steepest
    descent of start + entries per unit of effort from its derivative (return_sensitivities=True returns it); the step along it is
    found on the window rule itself, evaluated at the means moved through the linearised dynamics -- the probability is not
    linearised -- by doubling and then closing a bracket (include/mpcx.h).  A row at or below target_p gets du = 0; a row without a
    direction (the same object twice) is status 4, one that runs out of evaluations 8 while doubling and 5 while closing.  The
    covariances are held as given and the manoeuvre is not flown again here.  An empty list returns empty arrays without a library
    call.  devices=[d0, d1, ...]: contiguous blocks of the list's rows on several devices, written in place, the bits of one device."""
    solve = _check_solve(target_p, tol, max_eval)
    pairs, half, how = _window_problem(pairs, radius, Y, U, units, span, consts, P, half_window, panels, ns, cat, who, mu)
    how.update(_model(include_drag, include_J2, atmosphere, max_step), **solve)
    out = _window_arrays(pairs.shape[0], how, return_sensitivities)
    if len(pairs):
        dispatch(_avoidance_window_call, [pairs, half], out, device, devices, **how)
    return AvoidanceWindowResult(pairs, out["out"], out["du"], out["sens"], out["status"])


def _avoidance_window_call(pairs, half, *, device, slot, out, rows, cols, mu, panels, who, flags, max_step, atmosphere, target_p, tol, max_eval):
    """one block of the list's rows on context (device, slot), into `out` (the block's views)"""
    pairs, half = _ffi.as_f64(pairs), _ffi.as_f64(half)
    _ffi.call("mpcx_avoidance_window", _context(device, slot, flags, atmosphere),
              *_window_args(pairs, half, rows, cols, mu, panels, who, flags, max_step), target_p, tol, max_eval,
              _ffi.dptr(out["out"]), _ffi.dptr(out["du"]), _ffi.dptr_opt(out.get("sens")), _ffi.iptr(out["status"]))


# ---- the window manoeuvre flown, re-evaluated and corrected (include/mpcx.h: mpcx_avoidance_window_refine;
# csrc/avoidance_window_refine.hip)
class AvoidanceWindowRefineResult(AvoidanceWindowResult):
    """AvoidanceWindowResult of the last accepted solve -- p0 is pass 0's figure, du the total change from the given U, evals summed
    over the passes -- with the answer as flown: Y_flown (n, NS, 7, K) every row's own last flight (a slot that does not move is a
    copy of the given trajectory), P_flown (n, NS, K, 6, 6) the covariances of that flight or None (recov), p_history and t_history
    (rounds + 2, n) each pass's window figure start + entries and the time it was taken about (pass 0: the given list; a row that
    does not fly repeats both), p_predicted (rounds + 1, n) each solve's p1 (NaN where nothing was solved), rounds_done (n,) int32
    the last pass whose solve was accepted (-1: none, or the row does not fly).  A row whose later flight, linearisation, tracking or
    solve failed keeps its earlier du and reports the failure in status (apply raises for it as for any status that is not 0; U + du
    is there to be taken)."""

    def __init__(self, pairs, out, du, sens, status, Y_flown, P_flown, p_history, t_history, p_predicted, rounds_done):
        super().__init__(pairs, out, du, sens, status)
        self.Y_flown, self.P_flown, self.p_history, self.t_history = Y_flown, P_flown, p_history, t_history
        self.p_predicted, self.rounds_done = p_predicted, rounds_done

    def __repr__(self):
        return f"AvoidanceWindowRefineResult(pairs={len(self.pairs)}, passes={len(self.p_history)})"


def avoidance_window_refine(pairs, target_p, radius, Y, U, units, span, consts, P, half_window, rounds=2, track=None, max_shift=None,
                            recov=False, q=None, prop_max_step=1e-3, panels=DEFAULT_PANELS, ns=None, cat=None, who="i",
                            tol=_ffi.AW_DEFAULT_TOL, max_eval=_ffi.AW_DEFAULT_MAX_EVAL, include_drag=False, include_J2=False,
                            atmosphere=None, max_step=DEFAULT_MAX_STEP, mu=None, return_sensitivities=False, return_covariances=True,
                            device=0, devices=None):
    """avoidance_window, then `rounds` times on the device: fly U + du through the nonlinear dynamics (include_drag / include_J2 /
    atmosphere are the model of the flight and of the linearisation; prop_max_step the flight's step limit), take the window figure
    again on what was flown, linearise about it and solve again for the TOTAL change from the given U -- and once more fly and look
    -> AvoidanceWindowRefineResult, the answer as flown.  All other arguments as avoidance_window takes them.  rounds = 0 is
    avoidance_window followed by one flight and one figure.  track = (M, T0, T1): every row's time is found again in every pass by
    screen_track of the row AS GIVEN on the pass's trajectories over linspace(T0, T1, M), at most max_shift seconds away (None or
    <= 0: unlimited); a row that loses its event is frozen with MPCX_ST_BADK = 9.  track = None: every row keeps its given time.
    recov=True: the covariances of every object that moves are propagated again along its flight (covariance's chain from P[o][0]
    and q, a scalar or (S,), None: 0) and returned as P_flown (return_covariances=False: not returned); False: P is held as given.
    Rows are independent -- every row flies its own copy of the objects that move for it, two rows that move one satellite do not see
    each other -- so nothing is installed anywhere and the call has a block form: devices=[d0, d1, ...] deals contiguous blocks of
    the list's rows to several devices, written in place, the bits of one device.  An empty list returns empty arrays without a
    library call."""
    solve = _check_solve(target_p, tol, max_eval)
    rounds, prop_max_step = _check_rounds(rounds, prop_max_step)
    if track is None:
        grid = (0, 0.0, 0.0, 0.0)
    else:
        if np.ndim(track) != 1 or len(track) != 3:
            raise ValueError(f"track: expected None or (M, T0, T1), got {track!r}")
        grid = (*_check_grid(*track), _check_max_shift(max_shift))
    pairs, half, how = _window_problem(pairs, radius, Y, U, units, span, consts, P, half_window, panels, ns, cat, who, mu)
    (S, _, K), n, recov = how["rows"][0].shape, pairs.shape[0], bool(recov)
    out = _window_arrays(n, how, return_sensitivities)
    NS = out["du"].shape[1]
    out.update(rounds_done=np.full(n, -1, dtype=np.int32), Y_flown=_ffi.result_pool.take((n, NS, 7, K)),
               P_flown=_ffi.result_pool.take((n, NS, K, 6, 6)) if recov and return_covariances else None)
    hist = dict(p_history=np.empty((rounds + 2, n)), t_history=np.empty((rounds + 2, n)), p_predicted=np.empty((rounds + 1, n)))
    how.update(_model(include_drag, include_J2, atmosphere, max_step), **solve, prop_max_step=prop_max_step, rounds=rounds, grid=grid,
               recov=int(recov), q=_check_q(q, S) if recov else None)
    if n:
        dispatch(_avoidance_window_refine_call, [pairs, half], dict(out, **{k: (a, 1) for k, a in hist.items()}), device, devices, **how)
    return AvoidanceWindowRefineResult(pairs, out["out"], out["du"], out["sens"], out["status"], out["Y_flown"], out["P_flown"],
                                       hist["p_history"], hist["t_history"], hist["p_predicted"], out["rounds_done"])


def _avoidance_window_refine_call(pairs, half, *, device, slot, out, rows, cols, mu, panels, who, flags, max_step, atmosphere, target_p, tol,
                                  max_eval, prop_max_step, rounds, grid, recov, q):
    """one block of the list's rows on context (device, slot), into `out` (the block's views; a block's columns of the histories go
    through contiguous temporaries)"""
    pairs, half = _ffi.as_f64(pairs), _ffi.as_f64(half)
    ctx = _context(device, slot, flags, atmosphere)
    hist = {k: out[k] if out[k].flags.c_contiguous else np.empty(out[k].shape) for k in ("p_history", "t_history", "p_predicted")}
    _ffi.call("mpcx_avoidance_window_refine", ctx, *_window_args(pairs, half, rows, cols, mu, panels, who, flags, max_step), target_p, tol,
              max_eval, prop_max_step, rounds, *grid, recov, _ffi.dptr_opt(q), _ffi.dptr(out["out"]), _ffi.dptr(out["du"]),
              _ffi.dptr_opt(out.get("sens")), _ffi.iptr(out["status"]), _ffi.iptr(out["rounds_done"]), _ffi.dptr(out["Y_flown"]),
              _ffi.dptr_opt(out.get("P_flown")), _ffi.dptr(hist["p_history"]), _ffi.dptr(hist["t_history"]), _ffi.dptr(hist["p_predicted"]))
    for k, a in hist.items():
        if a is not out[k]:
            out[k][...] = a


# ---- all of a satellite's encounters under its thrust limit (include/mpcx.h: mpcx_avoidance_joint; csrc/avoidance_joint.hip)
class AvoidanceJointResult:
    """Per satellite (S,): du (S, 3, K) the thrust change in the plan's own units (zero for a satellite without rows and for nodes
    past ns), cost (1/2 sum D |du|^2), dv (sum of w_m |da_m|, m/s), umax (the largest |ubar + du|, normalised), n_rows, n_active
    (rows with a positive multiplier), n_on_ball (nodes the thrust ball projects), iters, residual (final max |F|), status
    (int32 MPCX_ST_*; a satellite whose status is not 0 is NaN in all of them), tsens (S, 6, 3, K) the terminal sensitivities T_m
    or None.  Per row of `pairs` (n,): mover (0: object i moves, 1: object j), d0 the distance now, margin the linear margin
    q^T (m + dm) (to compare with the target), d1 the predicted distance sqrt((m + dm)^T W (m + dm)), lam the row's multiplier,
    dt the shift of the time of closest approach (s), row_status, rows (n, 3, K) the a_p or None, and coupled (n,) bool: the
    row's object that does NOT move is itself moved by another row of the list, which this row's prediction ignores."""

    def __init__(self, pairs, mover, du, sat_out, row_out, rows, tsens, status, row_status, coupled):
        self.pairs, self.mover, self.du, self.rows, self.tsens, self.status, self.row_status, self.coupled = \
            pairs, mover, du, rows, tsens, status, row_status, coupled
        self.cost, self.dv, self.umax = sat_out[:, _ffi.AJ_COST], sat_out[:, _ffi.AJ_DV], sat_out[:, _ffi.AJ_UMAX]
        self.n_rows, self.n_active, self.n_on_ball = sat_out[:, _ffi.AJ_ROWS], sat_out[:, _ffi.AJ_ACTIVE], sat_out[:, _ffi.AJ_ONBALL]
        self.iters, self.residual = sat_out[:, _ffi.AJ_ITERS], sat_out[:, _ffi.AJ_RESIDUAL]
        self.d0, self.margin, self.d1 = row_out[:, _ffi.AR_D0], row_out[:, _ffi.AR_MARGIN], row_out[:, _ffi.AR_DIST]
        self.lam, self.dt = row_out[:, _ffi.AR_LAMBDA], row_out[:, _ffi.AR_DT]
        self.sat_out, self.row_out = sat_out, row_out

    def __repr__(self):
        return f"AvoidanceJointResult(pairs={len(self.pairs)}, satellites={len(self.du)})"

    def apply(self, U):
        """a copy of the plan thrust U (S, 3, K) with every satellite's du added; raises for a satellite whose status is not 0"""
        U = np.array(U, dtype=np.float64)
        if U.shape != self.du.shape:
            raise ValueError(f"U: expected {self.du.shape} plan thrust, got {U.shape}")
        bad = np.flatnonzero(self.status != 0)
        if len(bad):
            s = int(bad[0])
            raise ValueError(f"satellite {s} has no manoeuvre: {_ffi.STATUS_TEXT.get(int(self.status[s]), int(self.status[s]))}")
        return U + self.du


def _check_mover(who, n, against_catalogue):
    """who = 'i', 'j' or an (n,) array of 0 / 1 -> mover (n,) int32"""
    if isinstance(who, str):
        if who not in ("i", "j"):
            raise ValueError(f"who: expected 'i', 'j' or an ({n},) array of 0 (object i moves) / 1 (object j), got {who!r}")
        mover = np.full(n, _WHO[who], dtype=np.int32)
    else:
        w = np.asarray(who)
        if w.shape != (n,) or not np.isin(w, (0, 1)).all():
            raise ValueError(f"who: expected 'i', 'j' or an ({n},) array of 0 (object i moves) / 1 (object j), got shape {w.shape}")
        mover = np.ascontiguousarray(w, dtype=np.int32)
    if against_catalogue and mover.any():
        raise ValueError("who: against a catalogue only the satellite can manoeuvre (who='i', or all 0)")
    return mover


def _coupled(pairs, mover, against_catalogue):
    """rows whose object that does not move is moved by another row"""
    n = len(pairs)
    if against_catalogue or n == 0:
        return np.zeros(n, dtype=bool)
    at = np.arange(n)
    moving, other = pairs[at, mover], pairs[at, 1 - mover]
    return np.isin(other, moving)


def _joint_problem(pairs, target, Y, U, units, span, consts, ns, P, cat, who, u_max, hold_terminal, tol, max_iter, mu):
    """the checks avoidance_joint and avoidance_refine share -> the keywords their block functions share, from pairs to max_iter"""
    if not (np.ndim(tol) == 0 and np.isfinite(tol) and tol > 0.0):
        raise ValueError(f"tol: need a positive finite number, got {tol}")
    if not (np.ndim(max_iter) == 0 and int(max_iter) == max_iter and max_iter >= 1):
        raise ValueError(f"max_iter: need an integer >= 1, got {max_iter}")
    pairs, Y, U, units, span, consts, ns, P, cols, mu = _encounter_problem(pairs, target, Y, U, units, span, consts, ns, P, cat, mu)
    mover = _check_mover(who, pairs.shape[0], cols is not None)
    if u_max is not None:
        u_max = _per_row(u_max, Y.shape[0], "u_max", "normalised thrust limits")
        if not (u_max > 0.0).all():
            raise ValueError("u_max: need positive limits (inf: no ball)")
    return dict(pairs=pairs, mover=mover, rows=(Y, U, units, span, consts, ns, P, u_max), cols=cols, mu=mu, target=float(target),
                hold=1 if hold_terminal else 0, tol=float(tol), max_iter=int(max_iter))


def _joint_arrays(S, K, n, return_rows, return_terminal):
    """the result arrays of the joint call: what the library writes for every satellite and every row of the list"""
    return dict(du=np.zeros((S, 3, K)), sat_out=np.zeros((S, _ffi.NAJ)), row_out=np.zeros((n, _ffi.NAR)),
                rows=np.zeros((n, 3, K)) if return_rows else None, tsens=np.zeros((S, 6, 3, K)) if return_terminal else None,
                sat_status=np.zeros(S, dtype=np.int32), row_status=np.zeros(n, dtype=np.int32))


def avoidance_joint(pairs, target, Y, U, units, span, consts, ns=None, P=None, cat=None, who="i", u_max=None, hold_terminal=True,
                    tol=_ffi.AJ_DEFAULT_TOL, max_iter=_ffi.AJ_DEFAULT_MAX_ITER, include_drag=False, include_J2=False, atmosphere=None,
                    max_step=DEFAULT_MAX_STEP, mu=None, return_rows=False, return_terminal=False, device=0, devices=None):
    """One thrust change per manoeuvring satellite that opens ALL of its listed close approaches to `target` at once, stays inside
    its thrust ball |U + du| <= u_max at every node and, with hold_terminal, leaves the plan's last position and velocity where they
    were to first order -> AvoidanceJointResult.  pairs, target, Y, U, units, span, consts, ns, P, cat and the model as `avoidance`
    takes them; who = "i", "j" or an (n,) array of 0 / 1: which object of each pair moves (exactly one; against a catalogue the
    satellite).  u_max: a scalar or (S,) normalised thrust limits, None: no ball.  A satellite's rows are the pairs it moves for, at
    most 8; every row is the tangent half-plane of its target ellipse, so a met row is at or beyond the target to first order, and
    rows already beyond it stay in the problem.  The device solves the strictly convex problem per satellite by a semismooth Newton
    iteration to max |F| <= tol (include/mpcx.h).  return_rows / return_terminal: the rows a_p (n, 3, K) and the terminal
    sensitivities (S, 6, 3, K).  An empty list returns zeros without a library call.  devices=[d0, d1, ...]: contiguous blocks of
    satellites on several devices (every device holds the whole plan and list), written in place, the bits of one device."""
    how = _joint_problem(pairs, target, Y, U, units, span, consts, ns, P, cat, who, u_max, hold_terminal, tol, max_iter, mu)
    how.update(_model(include_drag, include_J2, atmosphere, max_step))
    (S, _, K), n = how["rows"][0].shape, len(how["pairs"])
    out = _joint_arrays(S, K, n, return_rows, return_terminal)
    if n:
        dispatch(_avoidance_joint_call, [np.arange(S)], None, device, devices, whole=out, **how)
    return AvoidanceJointResult(*_joint_result(how, out))


def _joint_result(how, out):
    """AvoidanceJointResult's arguments from the problem and the result arrays"""
    return (how["pairs"], how["mover"], out["du"], out["sat_out"], out["row_out"], out["rows"], out["tsens"], out["sat_status"], out["row_status"],
            _coupled(how["pairs"], how["mover"], how["cols"] is not None))


def _joint_args(pairs, mover, rows, cols, mu, target, hold, tol, max_iter, flags, max_step):
    """the arguments the joint calls share, from n to max_iter"""
    Y, U, units, span, consts, ns, P, u_max = rows
    return (len(pairs), _ffi.dptr(pairs), _ffi.iptr(mover), *_plan_args(Y, U, units, span, consts, ns, flags, max_step), _ffi.dptr_opt(P),
            *_side_args(cols, 1), mu, target, _ffi.dptr_opt(u_max), hold, tol, max_iter)


def _joint_outputs(out):
    """the result arrays of _joint_arrays as the library takes them"""
    return (_ffi.dptr(out["du"]), _ffi.dptr(out["sat_out"]), _ffi.dptr(out["row_out"]), _ffi.dptr_opt(out["rows"]), _ffi.dptr_opt(out["tsens"]),
            _ffi.iptr(out["sat_status"]), _ffi.iptr(out["row_status"]))


def _avoidance_joint_call(index, *, device, slot, out, pairs, mover, rows, cols, mu, target, hold, tol, max_iter, flags, max_step, atmosphere,
                          whole):
    """the block of satellites index[0] .. index[-1] on context (device, slot): the library writes the block's satellites and the
    rows they own into the whole result set `whole`, and nothing else of it"""
    _ffi.call("mpcx_avoidance_joint", _context(device, slot, flags, atmosphere),
              *_joint_args(pairs, mover, rows, cols, mu, target, hold, tol, max_iter, flags, max_step), int(index[0]), len(index), *_joint_outputs(whole))


# ---- the joint manoeuvre flown again, re-screened and corrected (include/mpcx.h: mpcx_avoidance_refine; csrc/avoidance_joint.hip)
class AvoidanceRefineResult(AvoidanceJointResult):
    """AvoidanceJointResult of the last accepted solve -- du is the total change from the given U -- with the answer as flown:
    Y_flown (S, 7, K) the last flight (the given trajectory for a satellite that does not fly), pairs_flown (n, 4) the last re-screen
    of the list on it, d0_history and tca_history (rounds + 2, n) each pass's distance in the target's metric and its time,
    terminal_history (rounds + 2, S) the largest normalised end-state difference from the given plan (0 for a satellite that does not
    fly), rounds_done (S,) int32 the last pass whose solve was accepted (-1: none, or no rows), and rhs_rows (n,) / rhs_term (S, 6)
    the last solve's right-hand sides or None.  A satellite whose later solve or flight failed keeps its earlier du and reports the
    failure in status (apply raises for it as for any status that is not 0; U + du is there to be taken)."""

    def __init__(self, joint, Y_flown, pairs_flown, d0_history, tca_history, terminal_history, rounds_done, rhs_rows, rhs_term):
        super().__init__(*joint)
        self.Y_flown, self.pairs_flown, self.d0_history, self.tca_history = Y_flown, pairs_flown, d0_history, tca_history
        self.terminal_history, self.rounds_done, self.rhs_rows, self.rhs_term = terminal_history, rounds_done, rhs_rows, rhs_term

    def __repr__(self):
        return f"AvoidanceRefineResult(pairs={len(self.pairs)}, satellites={len(self.du)}, passes={len(self.d0_history)})"


def avoidance_refine(pairs, target, Y, U, units, span, consts, M, T0, T1, rounds=3, ns=None, P=None, cat=None, who="i", u_max=None,
                     hold_terminal=True, tol=_ffi.AJ_DEFAULT_TOL, max_iter=_ffi.AJ_DEFAULT_MAX_ITER, include_drag=False, include_J2=False,
                     atmosphere=None, max_step=DEFAULT_MAX_STEP, prop_max_step=1e-3, mu=None, return_rows=False, return_terminal=False,
                     return_rhs=False, device=0, devices=None, track=False, max_shift=None):
    """avoidance_joint, then `rounds` times on the device: fly U + du through the nonlinear dynamics (include_drag / include_J2 /
    atmosphere are the model of the flight and of the linearisation; prop_max_step the flight's step limit), look at the LISTED pairs
    again on the grid linspace(T0, T1, M) (screen_pairs), linearise about what was flown and solve again -- the effort measured from
    the given U, the end state held to the given plan's, the multipliers of the last solve as the start -- and once more fly and
    re-screen -> AvoidanceRefineResult, the answer as flown.  All other arguments as avoidance_joint takes them.  rounds = 0 is
    avoidance_joint followed by one flight and re-screen.  A row whose other object is moved by another row (`coupled`) sees that
    object's new trajectory in every round.  An empty list returns zeros without a library call.  One device: every round needs every
    mover's new trajectory, so there is no block form and devices with more than one entry raises ValueError.
    track=True (mpcx_avoidance_refine_tracked): the re-screen is screen_track of the GIVEN list, so every row follows, in every pass,
    the encounter nearest the time it was given with -- what a list with several encounters of one pair (screen_events' rows) needs:
    under screen_pairs all rows of a pair read the pair's global minimum after the first flight, identical rows make the solve
    singular under the hold, and the other encounters are never looked at again.  max_shift (seconds; None or <= 0: unlimited): how
    far from its given time a row's encounter may be found; a row that loses its encounter reads (+inf, NaN), its mover's solve
    fails with MPCX_ST_BADK = 9 and the satellite is frozen with the manoeuvre it had.  max_shift is read only with track=True; with
    track=False nothing changes."""
    how = _joint_problem(pairs, target, Y, U, units, span, consts, ns, P, cat, who, u_max, hold_terminal, tol, max_iter, mu)
    pairs, Y = how["pairs"], how["rows"][0]
    (S, _, K), n = Y.shape, pairs.shape[0]
    rounds, prop_max_step = _check_rounds(rounds, prop_max_step)
    if devices is not None and len(devices) > 1:
        raise ValueError(f"devices: avoidance_refine runs on one device (every round needs every mover's new trajectory), got {len(devices)}")
    out = dict(_joint_arrays(S, K, n, return_rows, return_terminal), Y_flown=Y.copy(), pairs_flown=pairs.copy(),
               d0=np.zeros((rounds + 2, n)), tca=np.zeros((rounds + 2, n)), term=np.zeros((rounds + 2, S)), rounds_done=np.full(S, -1, dtype=np.int32),
               rhs_rows=np.zeros(n) if return_rhs else None, rhs_term=np.zeros((S, 6)) if return_rhs else None)
    how.update(_model(include_drag, include_J2, atmosphere, max_step), grid=_check_grid(M, T0, T1), prop_max_step=prop_max_step, rounds=rounds,
               track=_check_max_shift(max_shift) if track else None, whole=out)
    if n:
        dispatch(_avoidance_refine_call, [], None, device, devices, **how)
    return AvoidanceRefineResult(_joint_result(how, out), out["Y_flown"], out["pairs_flown"], out["d0"], out["tca"], out["term"], out["rounds_done"],
                                 out["rhs_rows"], out["rhs_term"])


def _avoidance_refine_call(*, device, slot, out, whole, pairs, mover, rows, cols, mu, target, hold, tol, max_iter, flags, max_step, atmosphere, grid,
                           prop_max_step, rounds, track=None):
    """the whole list and all satellites on context (device, slot), into `whole`; track = max_shift: the tracked re-screen"""
    name, mode = ("mpcx_avoidance_refine", ()) if track is None else ("mpcx_avoidance_refine_tracked", (track,))
    _ffi.call(name, _context(device, slot, flags, atmosphere), *_joint_args(pairs, mover, rows, cols, mu, target, hold, tol, max_iter, flags, max_step),
              *grid, prop_max_step, rounds, *mode, *_joint_outputs(whole), _ffi.dptr(whole["Y_flown"]), _ffi.dptr(whole["pairs_flown"]),
              _ffi.dptr(whole["d0"]), _ffi.dptr(whole["tca"]), _ffi.dptr(whole["term"]), _ffi.iptr(whole["rounds_done"]),
              _ffi.dptr_opt(whole["rhs_rows"]), _ffi.dptr_opt(whole["rhs_term"]))
