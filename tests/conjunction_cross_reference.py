"""numpy restatement of the cross screen (include/mpcx.h: mpcx_conjunction_cross_screen) -- a constellation's satellites against a
catalogue of foreign objects: conjunction_reference.pair_minima on the union [constellation; catalogue], of which only the pairs
(satellite, object) are kept -- and a generator of cases.  Test infrastructure: the product never imports it."""
import functools

import numpy as np

import conjunction_reference as R


class CrossScreen:
    """dmin, partner (a catalogue index), tca per satellite; Q, T (S, D): every pair's squared minimum distance (inf: no valid
    interval) and its time; pairs: all pairs with a valid interval, rows (i, j, d, t) sorted by (i, j)"""

    def pairs_within(self, threshold):
        return self.pairs[self.pairs[:, 2] <= threshold]


def screen_against(eph, cat, T0, T1):
    eph, cat = np.asarray(eph, dtype=np.float64), np.asarray(cat, dtype=np.float64)
    S, D = eph.shape[0], cat.shape[0]
    lo, hi, q, tq, _ = R.pair_minima(np.concatenate([eph, cat]), T0, T1)
    cross = (lo < S) & (S <= hi)                                     # lower index a satellite, higher an object: catalogue - satellite
    Q = np.full((S, D), np.inf); T = np.full((S, D), np.nan)
    Q[lo[cross], hi[cross] - S] = q[cross]; T[lo[cross], hi[cross] - S] = tq[cross]
    r = CrossScreen()
    j = np.argmin(Q, axis=1)                                         # the first minimum: the smaller catalogue index on a tie
    qmin = Q[np.arange(S), j]
    none = ~(qmin < np.inf)
    r.dmin = np.where(none, np.inf, np.sqrt(qmin))
    r.partner = np.where(none, -1, j).astype(np.int32)
    r.tca = np.where(none, np.nan, T[np.arange(S), j])
    i, k = np.nonzero(Q < np.inf)                                    # (row-major: sorted by (i, j))
    r.pairs = np.column_stack([i, k, np.sqrt(Q[i, k]), T[i, k]]).astype(np.float64).reshape(-1, 4)
    r.Q, r.T = Q, T
    return r


@functools.lru_cache(maxsize=None)
def case(S, D, M, seed=0, n=40):
    """S + D random LEO orbits over one revolution of the lowest one, the first S the constellation, the others the catalogue:
    trajectories with n nodes, their restated ephemerides on M instants and the restated cross screen.  Treat as read-only."""
    orb = R.random_orbits(S + D, seed + 1000 * S + 7 * D + M)
    T0, T1 = 0.0, 2 * np.pi / R.orbit_rate(orb).max()
    Y, units, span = R.trajectories(orb, n, (T0 - 1.0, T1 + 1.0))
    eph, status = R.ephemeris(Y, units, span, M, T0, T1)
    assert (status == 0).all()
    sat = dict(Y=Y[:S], units=units[:S], span=span[:S])
    cat = dict(cat_Y=Y[S:], cat_units=units[S:], cat_span=span[S:])
    return dict(orb=orb, S=S, D=D, M=M, T0=T0, T1=T1, sat=sat, cat=cat, eph=eph[:S], cat_eph=eph[S:],
                ref=screen_against(eph[:S], eph[S:], T0, T1))


def assert_no_ties_and_moving(c):
    """what the tolerances of the device tests assume of a case: every row's nearest object is nearer than the next one by far more
    than the rounding, and every (satellite, object) pair moves at >= 1 m/s relative to each other at every instant"""
    ref = c["ref"]
    if c["D"] > 1:
        q = np.sort(np.sqrt(ref.Q), axis=1)
        assert (q[:, 1] - q[:, 0] > 1e-3).all()
    w2 = sum((c["cat_eph"][None, :, k, :] - c["eph"][:, None, k, :]) ** 2 for k in (3, 4, 5))
    assert np.sqrt(w2.min()) >= 1.0
