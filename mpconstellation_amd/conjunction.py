"""Conjunction screening: the constellation on one clock, and the closest approach of every pair of satellites on it.

Everything else in the package works on one satellite in its own units (SatelliteScale: length = its start radius, time = its
own orbital period), so node k of two trajectories is two different instants in two different lengths, and nothing looks at two
satellites at once.  Here (include/mpcx.h, csrc/conjunction.hip: one screen kernel and one host path behind both screens):

  common_clock   resamples trajectories at M common instants in metres and m/s (cubic Hermite on the node positions and velocities);
  screen         the closest approach of every ordered pair over every grid interval -- per satellite the nearest other one, how
                 near and when, and with a threshold the list of pairs that come closer than it;
  screen_against the same for a constellation against a catalogue of foreign objects (debris, other operators' satellites): the
                 rectangle satellites x objects, not the square of the union;
  catalogue_trajectories   a catalogue given as state vectors at an epoch, propagated to trajectories for screen_against.

The device does all of it (4096 satellites are 8.4 M pairs times the grid); there is no host path."""
import numpy as np

from . import _ffi

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
    rows = np.arange(S)
    if devices is not None and len(devices) > 1:
        from .sharding import sharded_call
        parts = sharded_call(_screen_call, devices, [rows], out, **how)
    else:
        if devices is not None and len(devices) == 1:
            device = int(devices[0])
        parts = [_screen_call(rows, device=device, slot=0, out=out, **how)]
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
        traj = [a for N, (Y, units, span, ns) in zip(counts, sides)
                for a in (N, Y.shape[2], _ffi.iptr_opt(ns), _ffi.dptr(Y), _ffi.dptr(units), _ffi.dptr(span))]
        statuses[:len(sides)] = [np.zeros(N, dtype=np.int32) for N in counts]
        _ffi.call(name + "_traj", ctx, *traj, M, *tail, *[_ffi.iptr(st) for st in statuses[:len(sides)]])
    n = int(n_pairs[0])
    return pairs[:min(n, max_pairs)], n, statuses


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
