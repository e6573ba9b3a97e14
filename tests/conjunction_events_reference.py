"""numpy restatement of "every close approach of a listed pair" (include/mpcx.h: mpcx_conjunction_events).  Per grid interval the
(q_m, t_m) of conjunction_reference.pair_minima restricted to that interval alone -- pair_minima itself, called on the two instants
of the interval -- then the definition: interval m holds an event iff q_m < inf, q_m < q_m-1 and q_m <= q_m+1 with an absent
neighbour counting as inf; an edge event has no valid neighbour on the side where its time is the interval's end.  Test
infrastructure: the product never imports it."""
import functools

import numpy as np

import conjunction_reference as R
import conjunction_cross_reference as X

GAP = 1e-9                                                           # relative: what separates an event's q from its neighbours'


def interval_table(eph, T0, T1):
    """For every pair lo < hi of eph (S, 6, M), np.triu_indices order: q (P, M-1) the squared closest approach inside every grid
    interval alone (inf: an end of the interval is invalid for the pair) and t (P, M-1) its time.  d = p_hi - p_lo."""
    eph = np.asarray(eph, dtype=np.float64)
    S, _, M = eph.shape
    tg, _ = R.grid(M, T0, T1)
    lo, hi = np.triu_indices(S, 1)
    q = np.full((len(lo), M - 1), np.inf); t = np.full((len(lo), M - 1), np.nan)
    for m in range(M - 1):
        _, _, qm, tm, _ = R.pair_minima(eph[:, :, m:m + 2], tg[m], tg[m + 1])
        q[:, m], t[:, m] = qm, tm
    return lo, hi, q, t


def events_of(q, t, tg, threshold=None):
    """one pair's events from its intervals' (q, t) and the grid instants tg -> (interval, distance, time, edge) arrays, in
    ascending interval order; threshold (m; None or <= 0: all) is applied to the events, sqrt(q) <= threshold"""
    left = np.concatenate([[np.inf], q[:-1]]); right = np.concatenate([q[1:], [np.inf]])
    event = (q < np.inf) & (q < left) & (q <= right)
    edge = (~(left < np.inf) & (t == tg[:-1])) | (~(right < np.inf) & (t == tg[1:]))
    d = np.sqrt(q)
    if threshold is not None and threshold > 0.0:
        event &= d <= threshold
    m = np.flatnonzero(event)
    return m, d[m], t[m], edge[m]


def assert_gaps(q, intervals):
    """the condition under which comparing event SETS with the device is sound: every event's q differs from each PRESENT
    neighbour's by at least GAP relative, so that rounding cannot move, add or drop an event.  Returns the smallest gap seen."""
    smallest = np.inf
    for m in intervals:
        for nb in (m - 1, m + 1):
            if 0 <= nb < len(q) and q[nb] < np.inf:
                gap = abs(q[nb] - q[m]) / q[m]
                assert gap >= GAP, (m, nb, q[m], q[nb])
                smallest = min(smallest, gap)
    return smallest


class PairEvents:
    """one listed pair's events in the restatement: interval, d, t, edge (arrays), and q, the pair's per-interval table"""

    def __init__(self, q, t, tg, threshold=None):
        self.q = q
        self.interval, self.d, self.t, self.edge = events_of(q, t, tg, threshold)
        self.count = len(self.interval)


def all_pairs(eph, T0, T1, threshold=None):
    """{(i, j), i < j: PairEvents} for every pair of one constellation"""
    tg, _ = R.grid(eph.shape[2], T0, T1)
    lo, hi, q, t = interval_table(eph, T0, T1)
    return {(int(i), int(j)): PairEvents(q[k], t[k], tg, threshold) for k, (i, j) in enumerate(zip(lo, hi))}


def against(eph, cat_eph, T0, T1, threshold=None):
    """{(satellite, object): PairEvents}: the pairs (i, S + j) of the union [eph; cat_eph], catalogue - satellite"""
    S = eph.shape[0]
    tg, _ = R.grid(eph.shape[2], T0, T1)
    lo, hi, q, t = interval_table(np.concatenate([eph, cat_eph]), T0, T1)
    return {(int(i), int(j) - S): PairEvents(q[k], t[k], tg, threshold) for k, (i, j) in enumerate(zip(lo, hi)) if i < S <= j}


def smallest_gap(ref):
    """assert_gaps over every pair of a restated scene -> the scene's smallest gap"""
    return min([assert_gaps(p.q, p.interval) for p in ref.values()] + [np.inf])


# ---------------------------------------------------------------- shared cases (computed once per shape; read-only)
@functools.lru_cache(maxsize=None)
def case(S, M, n=40, orbits=1.0):
    """conjunction_reference.case(S, M, n=n, orbits=orbits) and its restated events {(i, j): PairEvents} -> (case, events)"""
    c = R.case(S, M, n=n, orbits=orbits)
    return c, all_pairs(c["eph"], c["T0"], c["T1"])


@functools.lru_cache(maxsize=None)
def cross_case(S, D, M):
    c = X.case(S, D, M)
    return c, against(c["eph"], c["cat_eph"], c["T0"], c["T1"])
