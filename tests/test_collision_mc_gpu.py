"""The Monte Carlo collision probability on the device (csrc/collision_mc.hip): the draws and the scan against their numpy restatement
(collision_mc_reference.py), the flight against the public propagate_batch, counts, chunks and bit-for-bit repeatability, and the
sampled figures against the linearised ones they were built to confront (covariance, covariance_thrust, collision_probability,
collision_probability_window) on the planted scenes of collision_mc_scenes.py.

Tolerances.  Draws: collision_mc_reference.normal_bound (two libms' log and sincos) pushed through L and the Gates frame.  Scan: the
restatement is fed the DEVICE's trajectories, so only rounding separates the two: 1e-6 m on distances of tens of metres between
positions of 7e6 m (their Hermite differs by about 2e-9 m per operation; the interval's Newton steps amplify that by the inverse
curvature).  Truth: 4 standard errors of the sampled figure plus 3 x the models' own gap measured at N = 2^20
(profiles/collision_mc.txt, collision_mc_scenes.GAP_*)."""
import numpy as np
import pytest

import collision_mc_reference as M
import collision_mc_scenes as SC
import collision_reference as C
import collision_window_reference as W

pytestmark = pytest.mark.gpu


def bits(r):
    return tuple(np.ascontiguousarray(x).tobytes() for x in (r.p_hit, r.se_hit, r.start, r.entries, r.se_bound, r.excess, r.window, r.n_ok, r.counts,
                                                             r.status))


def draw_case(n, K, ragged=True):
    """n + 1 satellites of test_covariance_thrust_gpu.thrust_case (circular LEO orbits over 2000 s; ragged counts, the first is 2;
    thrust nodes at zero -- the first and the last among them -- and at half of u_off; garbage behind the counts; execution rows and
    mass variances that differ by satellite) and the rows (r, r + 1, ., 1000 s) with windows of +-100 s"""
    from test_covariance_thrust_gpu import thrust_case
    c = thrust_case(n + 1, K, ragged)
    c["pairs"] = np.array([[r, r + 1, 0.0, 1000.0] for r in range(n)], dtype=np.float64)
    c["counts"] = np.full(n + 1, K) if c["ns"] is None else c["ns"]
    return c


def run(c, N, **kw):
    from mpconstellation_amd import collision_probability_mc
    kw = {**dict(execution=c.get("ex"), mass_var0=c.get("mv"), ns=c.get("ns")), **kw}
    return collision_probability_mc(c["pairs"], c.get("radius", 5.0), c["Y"], c["U"], c["units"], c["span"], c["consts"], c.get("P0", C.P0_TEST),
                                    c.get("half_window", 100.0), N, **kw)


@pytest.mark.parametrize("n,K,N", [(1, 5, 64), (3, 8, 65), (2, 31, 130)])
def test_draws_against_the_restatement(n, K, N):
    """the first column of Y_samples and U_samples of every (row, slot, sample) inside the computed bound of the restated draws, with
    execution errors and with execution=None (then U_samples is the plan's table, to the bit); columns past a count are zero"""
    c = draw_case(n, K)
    seed = 1234567 + (9 << 40)
    for ex in (c["ex"], None):
        res = run(c, N, seed=seed, execution=ex, return_trajectories=True)
        assert (res.status == 0).all() and res.Y_samples.shape == (n, 2, N, 7, K)
        worst = 0.0
        for r in range(n):
            for sl in range(2):
                o = int(c["pairs"][r, sl]); nn = int(c["counts"][o])
                ok, y0, by = M.draw_initial(c["Y"][o, :, 0], c["units"][o], C.P0_TEST, c["mv"][o], np.arange(N), o, 0, seed)
                u, bu = M.draw_thrust(c["U"][o], nn, None if ex is None else ex[o], np.arange(N), o, 0, seed)
                assert ok
                dy, du = np.abs(res.Y_samples[r, sl, :, :, 0] - y0), np.abs(res.U_samples[r, sl] - u)
                assert (dy <= by).all() and (du <= bu).all(), (r, sl, (dy / by).max())
                worst = max(worst, (dy / by).max(), (du[bu > 0.0] / bu[bu > 0.0]).max() if (bu > 0.0).any() else 0.0)
                assert (res.U_samples[r, sl, :, :, nn:] == 0.0).all() and (res.Y_samples[r, sl, :, :, nn:] == 0.0).all()
                off = np.linalg.norm(c["U"][o, :, :nn], axis=0) <= (0.0 if ex is None else ex[o, 4])
                assert np.array_equal(res.U_samples[r, sl][:, :, :nn][:, :, off], np.broadcast_to(c["U"][o, :, :nn][:, off], (N, 3, int(off.sum()))))
                if ex is None:
                    assert np.array_equal(res.U_samples[r, sl, :, :, :nn], np.broadcast_to(c["U"][o, :, :nn], (N, 3, nn)))
                elif (~off).any():
                    assert (res.U_samples[r, sl][:, :, :nn][:, :, ~off] != c["U"][o, :, :nn][:, ~off][None]).any()
        print(f"n {n} K {K} N {N} execution {'on' if ex is not None else 'None'}: worst |device - restated| / bound {worst:.3f}")


def test_flight_is_the_public_propagate_batch():
    """Y_samples of every sample equals propagate_batch from that sample's initial state under its executed thrust table, bit for bit"""
    from mpconstellation_amd import propagate_batch, _ffi
    n, K, N = 3, 8, 33
    c = draw_case(n, K)
    res = run(c, N, seed=5, include_J2=True, return_trajectories=True)
    obj = c["pairs"][:, :2].astype(int)                                   # (n, 2)
    y0 = res.Y_samples[:, :, :, :, 0].reshape(-1, 7)
    each = lambda a: np.repeat(a[obj].reshape(n * 2, *a.shape[1:]), N, axis=0)
    tf = each((c["span"][:, 1] - c["span"][:, 0]) / c["units"][:, 1])
    counts = each(c["counts"]).astype(np.int32)
    y, st, _ = propagate_batch(y0, tf, each(c["consts"]), (_ffi.CTRL_SEQUENCE, res.U_samples.reshape(-1, 3, K), K, 1.0), counts, include_J2=True,
                               max_step=1e-3, Kus=counts)
    assert (st == 0).all() and (res.status == 0).all()
    assert np.array_equal(y, res.Y_samples.reshape(-1, 7, K))


def slow_case(n_rows=2):
    """collision_mc_scenes.slow_pair with a second row of the same pair about another time, a shorter window and the objects swapped"""
    sc = SC.slow_pair()
    sc["pairs"] = np.array([[0.0, 1.0, 50.0, 3000.0], [1.0, 0.0, 50.0, 4100.0]])[:n_rows]
    sc["half_window"] = np.array([2000.0, 700.0])[:n_rows]
    return sc


SCAN_TOL = 1e-6                                                           # metres (the file's docstring)


@pytest.mark.parametrize("scan", [1, 64, 100])
def test_scan_against_the_restatement_on_the_devices_trajectories(scan):
    """per-sample records against collision_mc_reference.scan_pair fed Y_samples: inside_start, entries and hit equal for every sample
    that is not marginal (an end distance, an interval minimum or dmin within SCAN_TOL of R), dmin within SCAN_TOL, t_min within a
    second; at most 1 % marginal"""
    sc = slow_case()
    sc["radius"] = np.array([30.0, 40.0])                                # (R = 70 m: hits and misses in comparable numbers)
    N = 150
    res = run(sc, N, seed=11, scan=scan, return_samples=True, return_trajectories=True)
    assert (res.status == 0).all() and (res.samples[:, :, M.NMS - 1] == 0.0).all()
    R = sc["radius"].sum()
    marginal = 0
    for r, row in enumerate(sc["pairs"]):
        i, j = int(row[0]), int(row[1])
        ta, tb = M.window(row[3], sc["half_window"][r], sc["span"][i], sc["span"][j])
        assert np.array_equal(res.window[r], [ta, tb])
        for s in range(N):
            (dmin, tmin, ins, ent), q_ends, qm = M.scan_pair(res.Y_samples[r, 0, s], 61, sc["span"][i], sc["units"][i], res.Y_samples[r, 1, s], 61,
                                                            sc["span"][j], sc["units"][j], ta, tb, R, scan)
            near = min(np.abs(np.sqrt(q_ends) - R).min(), np.abs(np.sqrt(qm) - R).min())
            got = res.samples[r, s]
            assert abs(got[0] - dmin) <= SCAN_TOL, (r, s, got[0], dmin)
            if near <= SCAN_TOL:
                marginal += 1
                continue
            assert (got[2], got[3]) == (ins, ent), (r, s, got, ins, ent)
            assert abs(got[1] - tmin) <= 1.0, (r, s, got[1], tmin)        # (seconds, in windows of thousands: a flat minimum moves its time)
    hits = ((res.samples[:, :, 2] + res.samples[:, :, 3]) >= 1).sum(axis=1)
    print(f"scan {scan}: {marginal} marginal of {2 * N}; hits per row {hits.tolist()}, entries {res.samples[:, :, 3].sum(axis=1).tolist()}")
    assert marginal <= 0.01 * 2 * N and 0 < hits.sum() < 2 * N


def test_counts_are_the_sums_of_the_samples_and_chunks_change_no_bit():
    """counts = the sums over `samples`, exactly; out = the counts' figures; max_flights forcing three chunks (and one sample per chunk)
    gives the bits of one chunk, optional outputs included; hit = inside_start or entries >= 1 per sample"""
    sc = slow_case()
    N = 100
    one = run(sc, N, seed=21, return_samples=True, return_trajectories=True)
    assert np.array_equal(one.counts, M.counts_of(one.samples)) and (one.counts[:, 0] == N).all() and (one.counts[:, 1] == 0).all()
    out = M.out_of(one.counts, one.window[:, 0], one.window[:, 1])
    got = np.column_stack([one.p_hit, one.se_hit, one.start, one.entries, one.se_bound, one.excess, one.window, one.n_ok])
    assert np.allclose(got, out, rtol=4e-16, atol=0.0) and np.array_equal(one.n_ok, [N, N])
    for max_flights in (2 * 2 * 34, 1):                                  # 34 samples per chunk: 34 + 34 + 32; one sample per chunk
        three = run(sc, N, seed=21, return_samples=True, return_trajectories=True, max_flights=max_flights)
        assert bits(three) == bits(one) and np.array_equal(three.samples, one.samples)
        assert np.array_equal(three.Y_samples, one.Y_samples) and np.array_equal(three.U_samples, one.U_samples)


def test_a_list_longer_than_a_grid_dimension():
    """66 000 rows (more than the 65 535 a grid's y and z dimensions take) of one pair, two samples, one sample per chunk: every row
    has the first row's counts -- the same objects, the same worlds"""
    sc = slow_case(1)
    n = 66000
    res = run(dict(sc, pairs=np.repeat(sc["pairs"], n, axis=0), half_window=2000.0), 2, seed=5)
    assert (res.status == 0).all() and (res.counts == res.counts[0]).all() and res.counts[0, 0] == 2 and (res.n_ok == 2.0).all()
    assert np.array_equal(res.window, np.broadcast_to([1000.0, 5000.0], (n, 2)))


def test_same_bits():
    """a row alone and inside a list; devices=[0, 0]; a second context; the _dev call over a workspace and results filled with garbage;
    with and without the optional outputs; the same seed twice; a different seed differs; a satellite shared by two rows has identical
    Y_samples in both; the catalogue form of the same objects: the satellite's trajectories to the bit -- the catalogue object draws
    from side 1, so the figures agree within sampling error, not to the bit"""
    import torch
    from mpconstellation_amd import conjunction as cj, _ffi
    from dev_solve import dev, filled, _p, _stream
    sc = slow_case()
    ex = np.array([1e-4, 0.02, 1e-4, 0.01745, 1e-3])
    sc["U"] = 1e-4 * np.random.default_rng(1).standard_normal((2, 3, 61))
    sc["U"][1] = 0.0                                                     # (object 1 is the catalogue's below: no thrust)
    N = 64
    kw = dict(seed=77, execution=ex, mass_var0=1e-6)
    full = run(sc, N, return_samples=True, return_trajectories=True, **kw)
    again, plain = run(sc, N, return_samples=True, return_trajectories=True, **kw), run(sc, N, **kw)
    assert (full.status == 0).all() and bits(full) == bits(again) == bits(plain) and np.array_equal(full.Y_samples, again.Y_samples)
    other = run(sc, N, return_trajectories=True, **{**kw, "seed": 78})
    assert bits(other) != bits(full) and not np.array_equal(other.Y_samples[:, :, :, :, 0], full.Y_samples[:, :, :, :, 0])
    # satellite 0 is slot 0 of row 0 and slot 1 of row 1: one world, one trajectory
    assert np.array_equal(full.Y_samples[0, 0], full.Y_samples[1, 1]) and np.array_equal(full.Y_samples[0, 1], full.Y_samples[1, 0])
    assert np.array_equal(full.U_samples[0, 0], full.U_samples[1, 1])
    for r in range(2):
        alone = dict(sc, pairs=sc["pairs"][r:r + 1], half_window=sc["half_window"][r:r + 1])
        one = run(alone, N, return_samples=True, return_trajectories=True, **kw)
        assert np.array_equal(one.samples[0], full.samples[r]) and np.array_equal(one.Y_samples[0], full.Y_samples[r])
        assert np.array_equal(one.counts[0], full.counts[r]) and one.p_hit.tobytes() == full.p_hit[r:r + 1].tobytes()
    two = run(sc, N, return_samples=True, return_trajectories=True, devices=[0, 0], **kw)
    assert bits(two) == bits(full) and np.array_equal(two.samples, full.samples) and np.array_equal(two.Y_samples, full.Y_samples)
    # a second context
    out = dict(out=np.empty((2, _ffi.NMC)), counts=np.zeros((2, _ffi.NMCC), dtype=np.int64), status=np.zeros(2, dtype=np.int32))
    rows = (sc["Y"], sc["U"], sc["units"], sc["span"], sc["consts"], None, cj._check_p0(sc["P0"], 2), cj._check_execution(ex, 2), np.full(2, 1e-6), sc["radius"])
    cj._collision_mc_call(sc["pairs"], sc["half_window"], device=0, slot=1, out=out, rows=rows, cols=None, scan=64, samples=N, seed=77, max_flights=0,
                          flags=0, prop_max_step=cj.DEFAULT_PROP_MAX_STEP, atmosphere=None)
    assert np.array_equal(out["counts"], full.counts) and out["out"].tobytes() == np.column_stack(
        [full.p_hit, full.se_hit, full.start, full.entries, full.se_bound, full.excess, full.window, full.n_ok]).tobytes()
    # the _dev call, every device buffer a torch tensor, workspace and results pre-filled
    lib, ctx = _ffi.load(), _ffi.context(0)
    wsb = int(lib.mpcx_collision_probability_mc_workspace_bytes(2, 2, 61, 0, 0, N, 2 * 2 * 30))
    assert 0 < wsb < int(lib.mpcx_collision_probability_mc_workspace_bytes(2, 2, 61, 0, 0, N, 0)) and wsb % 8 == 0
    ins = [dev(a) for a in (sc["pairs"], sc["Y"], sc["U"], sc["units"], sc["span"], sc["consts"], np.broadcast_to(sc["P0"], (2, 6, 6)),
                            np.broadcast_to(ex, (2, 5)), np.full(2, 1e-6), sc["radius"], sc["half_window"])]
    for fill in ("zero", "big", "nan+"):
        ws, dout, dsm = filled(wsb // 8, fill), filled(2 * _ffi.NMC, fill), filled(2 * N * _ffi.NMS, fill)
        dcn = torch.full((2, _ffi.NMCC), -7, dtype=torch.int64, device=ws.device)
        dst = torch.full((2,), -7, dtype=torch.int32, device=ws.device)
        rc = lib.mpcx_collision_probability_mc_dev(ctx, 2, _p(ins[0]), 2, 61, None, _p(ins[1]), _p(ins[2]), _p(ins[3]), _p(ins[4]), _p(ins[5]), 0,
                                                   cj.DEFAULT_PROP_MAX_STEP, _p(ins[6]), _p(ins[7]), _p(ins[8]), _p(ins[9]), 0, 0, None, None, None, None,
                                                   None, None, None, _p(ins[10]), 64, N, 77, 2 * 2 * 30, _p(dcn), _p(dout), _p(dst), _p(dsm), None, None,
                                                   _p(ws), _stream(torch))
        _ffi.check(rc, ctx, "mpcx_collision_probability_mc_dev")
        torch.cuda.synchronize()
        assert np.array_equal(dcn.cpu().numpy(), full.counts) and dout.cpu().numpy().tobytes() == out["out"].tobytes(), fill
        assert np.array_equal(dsm.cpu().numpy().reshape(2, N, _ffi.NMS), full.samples) and dst.cpu().numpy().tolist() == [0, 0], fill
    # the catalogue form: object 1 as a catalogue of one
    Nc = 2048
    cat = (sc["Y"][1:], sc["units"][1:], sc["span"][1:], sc["consts"][1:], sc["P0"][1:], sc["radius"][1:])
    rowc = dict(sc, pairs=np.array([[0.0, 0.0, 50.0, 3000.0]]), half_window=2000.0)
    a = run(dict(sc, pairs=sc["pairs"][:1], half_window=2000.0), Nc, return_trajectories=True, **kw)
    b = run(rowc, Nc, cat=cat, return_trajectories=True, **kw)
    assert b.status.tolist() == [0] and b.Y_samples.shape == (1, 1, Nc, 7, 61) and np.array_equal(b.Y_samples[0, 0], a.Y_samples[0, 0])
    assert np.array_equal(b.window, a.window) and b.counts[0, 0] == Nc
    se = np.hypot(a.se_hit[0], b.se_hit[0])
    print(f"all-pairs form P_HIT {a.p_hit[0]:.4f}, catalogue form {b.p_hit[0]:.4f}, difference {(a.p_hit[0] - b.p_hit[0]) / se:+.2f} combined SE")
    assert abs(a.p_hit[0] - b.p_hit[0]) <= 5.0 * se


def window_rule(sc, half, **model):
    from mpconstellation_amd import covariance, collision_probability_window
    P = covariance(sc["Y"], sc["units"], sc["span"], sc["consts"], sc["P0"], U=sc["U"], **model)
    win = collision_probability_window(sc["pairs"], sc["radius"], sc["Y"], sc["units"], sc["span"], P, half, panels=sc["panels"])
    assert (win.status == 0).all()
    return P, win


def test_truth_slow_pair():
    """collision_mc_scenes.slow_pair: the restated window rule (collision_window_reference on the device's covariance(P0)) lies in
    [0.03, 0.5]; at N = 16384 the sampled START + ENTRIES is within 4 SE_BOUND + 3 x GAP_SLOW_BOUND of the rule's, and the START
    columns within 4 SE + 3 x GAP_SLOW_START.  Measured at N = 2^20 (profiles/collision_mc.txt): see collision_mc_scenes.GAP_*."""
    sc = SC.slow_pair()
    P, win = window_rule(sc, sc["half_window"])
    ref, st = W.collision_probability_window(sc["pairs"], (sc["Y"], sc["units"], sc["span"], P, sc["radius"], None), sc["half_window"], sc["panels"])
    rule = ref[0, W.PW_START] + ref[0, W.PW_ENTRIES]
    assert st.tolist() == [0] and 0.03 <= rule <= 0.5 and abs(win.start[0] + win.entries[0] - rule) <= 1e-6 * rule
    N = 16384
    mc = run(sc, N, seed=101, mass_var0=None, execution=None)
    samp = mc.start[0] + mc.entries[0]
    se_start = np.sqrt(max(mc.start[0] * (1.0 - mc.start[0]), 1.0 / N) / N)
    print(f"slow pair: rule START {ref[0, W.PW_START]:.5f} + ENTRIES {ref[0, W.PW_ENTRIES]:.5f} = {rule:.5f}; sampled {mc.start[0]:.5f} + {mc.entries[0]:.5f} = "
          f"{samp:.5f} +- {mc.se_bound[0]:.5f}; P_HIT {mc.p_hit[0]:.5f} +- {mc.se_hit[0]:.5f}, EXCESS {mc.excess[0]:.5f}; counts {mc.counts[0].tolist()}")
    assert mc.status.tolist() == [0] and mc.counts[0, 1] == 0
    assert abs(samp - rule) <= 4.0 * mc.se_bound[0] + 3.0 * SC.GAP_SLOW_BOUND
    assert abs(mc.start[0] - ref[0, W.PW_START]) <= 4.0 * se_start + 3.0 * SC.GAP_SLOW_START
    assert mc.p_hit[0] <= samp and mc.excess[0] >= 0.0


def test_truth_fast_pair():
    """collision_mc_scenes.fast_pair (radii summing to 100 m, a position-only P0: positive semi-definite): the short-encounter Pc on
    covariance(P0), confirmed by collision_reference and inside the rule's R / sigma <= 2 domain; N = 32768, scan = 64, the half window
    of encounter_half_window: |P_HIT - Pc| <= 4 SE_HIT + 3 x GAP_FAST"""
    from mpconstellation_amd import covariance, collision_probability, encounter_half_window
    sc = SC.fast_pair()
    assert np.linalg.matrix_rank(sc["P0"]) == 3 and M.factor(sc["P0"])[0]
    P = covariance(sc["Y"], sc["units"], sc["span"], sc["consts"], sc["P0"])
    col = collision_probability(sc["pairs"], sc["radius"], sc["Y"], sc["units"], sc["span"], P)
    ref, st = C.collision_probability(sc["pairs"], (sc["Y"], sc["units"], sc["span"], P, sc["radius"], None))
    assert st.tolist() == [0] and col.status.tolist() == [0] and abs(col.pc[0] - ref[0, 0]) <= 1e-9 * ref[0, 0]
    assert 100.0 / col.sigma[0, 1] <= 2.0 and 0.005 <= col.pc[0] <= 0.2
    half = encounter_half_window(col, 100.0)
    N = 32768
    mc = run(dict(sc, half_window=half), N, seed=202, scan=64)
    print(f"fast pair: Pc {col.pc[0]:.5f} (sigma {col.sigma[0]} m, half window {half[0]:.4f} s); sampled P_HIT {mc.p_hit[0]:.5f} +- {mc.se_hit[0]:.5f}, "
          f"START {mc.start[0]:.2e}, ENTRIES {mc.entries[0]:.5f}; counts {mc.counts[0].tolist()}")
    assert mc.status.tolist() == [0] and mc.counts[0, 1] == 0
    assert abs(mc.p_hit[0] - col.pc[0]) <= 4.0 * mc.se_hit[0] + 3.0 * SC.GAP_FAST
    assert mc.excess[0] == 0.0                                           # a straight crossing at 8 km/s enters once


def test_reentry_excess():
    """collision_mc_scenes.reentry_pair: paths that pass inside and outside R several times.  Per sample hit = inside_start or entries >=
    1; EXCESS = START + ENTRIES - P_HIT exceeds 10 SE_BOUND; P_HIT <= the rule's START + ENTRIES + 4 SE; the sampled START + ENTRIES
    agrees with the rule's within 4 SE_BOUND + 3 x GAP_REENTRY_BOUND.  The first measurement of the bound's excess (printed; DESIGN.md
    section 8 records the N = 2^20 figure)."""
    sc = SC.reentry_pair()
    P, win = window_rule(sc, sc["half_window"])
    rule = win.start[0] + win.entries[0]
    N = 4096
    mc = run(sc, N, seed=303, scan=128, return_samples=True)
    s = mc.samples[0]
    hit = (s[:, 2] + s[:, 3]) >= 1.0
    samp = mc.start[0] + mc.entries[0]
    print(f"re-entry pair: rule START {win.start[0]:.4f} + ENTRIES {win.entries[0]:.4f} = {rule:.4f}; sampled {mc.start[0]:.4f} + {mc.entries[0]:.4f} = {samp:.4f} "
          f"+- {mc.se_bound[0]:.4f}; P_HIT {mc.p_hit[0]:.4f} +- {mc.se_hit[0]:.4f}; EXCESS {mc.excess[0]:.4f} = {mc.excess[0] / mc.se_bound[0]:.0f} SE_BOUND; "
          f"entries per sample: {np.bincount(s[:, 3].astype(int)).tolist()}")
    assert mc.status.tolist() == [0] and mc.counts[0, 1] == 0 and mc.counts[0, 5] == hit.sum() and mc.p_hit[0] == hit.sum() / N
    assert s[:, 3].max() >= 2 and mc.se_bound[0] > 0.0
    assert mc.excess[0] > 10.0 * mc.se_bound[0]
    assert mc.p_hit[0] <= rule + 4.0 * max(mc.se_hit[0], mc.se_bound[0])
    assert abs(samp - rule) <= 4.0 * mc.se_bound[0] + 3.0 * SC.GAP_REENTRY_BOUND


def test_execution_errors_against_covariance_thrust():
    """collision_mc_scenes.thrust_arc at K = 8, execution errors of 2 % and 1 degree (EXEC), N = 8192: the sample covariance of the last
    node from Y_samples against covariance_thrust's P, worst entry error over the largest entry in the orbit's units
    (test_covariance_thrust_host.mismatch's measure), inside 5 sqrt(2 / N) + 3 x 5.83e-4 (the sampling error of a covariance entry
    relative to the largest, and DESIGN.md's linearisation mismatch at K = 8).  The same statistic with execution=None in the sampler
    is outside that bound: the check sees the Gates draws."""
    from mpconstellation_amd import covariance_thrust
    a = SC.thrust_arc(8)
    N = 8192
    L, Tu = a["units"][0]
    d = 1.0 / np.array([L] * 3 + [L / Tu] * 3)
    P, st = covariance_thrust(a["Y"], a["units"], a["span"], a["consts"], a["P0"], a["U"], SC.EXEC, return_status=True)
    ref = P[0, -1] * d[:, None] * d[None, :]
    bound = 5.0 * np.sqrt(2.0 / N) + 3.0 * 5.83e-4
    stat = {}
    for label, ex in (("on", SC.EXEC), ("None", None)):
        c = dict(a, pairs=np.array([[0.0, 0.0, 0.0, 0.5 * a["span"][0, 1]]]), radius=1.0, half_window=10.0)
        mc = run(c, N, seed=404, scan=1, execution=ex, mass_var0=None, ns=None, return_trajectories=True)
        assert mc.status.tolist() == [0] and mc.counts[0, 1] == 0 and np.array_equal(mc.Y_samples[0, 0], mc.Y_samples[0, 1])
        x = mc.Y_samples[0, 0, :, :6, -1]
        stat[label] = np.abs(np.cov(x.T) - ref).max() / np.abs(ref).max()
    print(f"thrusting arc, last node: worst entry error over the largest entry {stat['on']:.4e} with execution errors, {stat['None']:.4e} with "
          f"execution=None; bound {bound:.4e}")
    assert st.tolist() == [0] and stat["on"] <= bound < stat["None"]


def test_failures_leave_the_neighbours_alone_and_failed_flights_are_counted():
    """every row status in one call -- a bad index, a time outside the span, h = 0 (BADK), a time unit of 0 (BADK: no tf), an indefinite
    P0, a negative execution entry, a negative mass variance, a radius that is not finite (NUMERIC), an object whose flights all fail
    (NUMERIC: no survivor), R = 0 (zeros, OK) -- NaN in out, zero in counts, the good rows between them bit for bit what they are in a
    list of their own.  A mass sigma of 100 % makes single flights fail (MPCX_ST_MASS): counted in FAILED, left out of the rest."""
    n, K, N = 12, 8, 48
    c = draw_case(12, K, ragged=False)
    S = n + 1
    P0 = np.broadcast_to(C.P0_TEST, (S, 6, 6)).copy()
    ex, mv, radius, units, Y = c["ex"].copy(), c["mv"].copy(), np.full(S, 5.0), c["units"].copy(), c["Y"].copy()
    pairs, half = c["pairs"].copy(), np.full(n, 100.0)
    pairs[:, 1] = pairs[:, 0]                                            # every row is (r, r): each object in one row only
    pairs[1, 0] = S; pairs[2, 3] = 1e6; half[3] = 0.0
    units[4, 1] = 0.0
    P0[5] = -P0[5]; ex[6, 1] = -0.1; mv[7] = -1e-6; radius[8] = np.inf
    Y[9, 6, 0] = -1.0; mv[9] = 0.0                                       # a negative mass: every flight ends with MPCX_ST_MASS
    radius[10] = 0.0
    mv[11] = 1.0                                                         # m0 = 1 + z: about 16 % of the flights fail
    U = c["U"].copy(); U[11] = 0.0                                       # (without thrust a small positive mass flies like any other)
    case = dict(c, pairs=pairs, half_window=half, radius=radius, units=units, Y=Y, U=U, P0=P0, ex=ex, mv=mv)
    res = run(case, N, seed=9, return_samples=True, return_trajectories=True)
    B, Nm = M.ST_BADK, M.ST_NUMERIC
    assert res.status.tolist() == [0, B, B, B, B, Nm, Nm, Nm, Nm, Nm, 0, 0]
    bad = res.status != 0
    assert np.isnan(res.p_hit[bad]).all() and np.isnan(res.window[bad]).all() and np.isfinite(res.p_hit[~bad]).all()
    assert (res.counts[bad] == 0).all()
    assert (res.samples[9, :, 4] == 1.0).all() and np.isnan(res.samples[9, :, 0]).all()
    assert res.counts[10].tolist() == [0] * 6 and res.p_hit[10] == 0.0 and res.n_ok[10] == 0.0 and np.array_equal(res.window[10], [900.0, 1100.0])
    assert (res.samples[10] == 0.0).all()
    failed = int(res.counts[11, 1])
    assert 1 <= failed <= N // 2 and res.counts[11, 0] == N and res.n_ok[11] == N - failed
    assert (res.samples[11, :, 4] != 0.0).sum() == failed and set(res.samples[11, :, 4].tolist()) <= {0.0, 1.0}
    m0 = res.Y_samples[11, 0, :, 6, 0]                                   # (a failed flight is NaN in Y_samples)
    assert np.isnan(m0).sum() == failed
    assert res.counts[11, 5] == N - failed and res.p_hit[11] == 1.0    # (an object against itself: always inside)
    good = dict(case, pairs=pairs[[0, 11]], half_window=half[[0, 11]])
    alone = run(good, N, seed=9, return_samples=True)
    assert np.array_equal(alone.counts, res.counts[[0, 11]]) and np.array_equal(alone.samples, res.samples[[0, 11]], equal_nan=True)
    assert alone.p_hit.tobytes() == res.p_hit[[0, 11]].tobytes()


def test_c_abi_refusals():
    from mpconstellation_amd import _ffi
    lib, ctx = _ffi.load(), _ffi.context(0)
    S, K, n, N = 2, 5, 1, 4
    d, i = _ffi.dptr, _ffi.iptr
    A = dict(pairs=np.array([[0.0, 1.0, 0.0, 0.5]]), Y=np.ones((S, 7, K)), units=np.ones((S, 2)), span=np.array([[0.0, 1.0]] * S), consts=np.ones((S, 8)),
             P0=np.zeros((S, 6, 6)), radius=np.ones(S), half=np.ones(n), out=np.full((n, _ffi.NMC), 7.0))
    counts, st = np.full((n, _ffi.NMCC), 7, dtype=np.int64), np.zeros(n, dtype=np.int32)
    catalogue = dict(cat_Y=np.ones((S, 7, K)), cat_units=np.ones((S, 2)), cat_span=np.array([[0.0, 1.0]] * S), cat_consts=np.ones((S, 8)),
                     cat_P0=np.zeros((S, 6, 6)), cat_radius=np.ones(S))

    def call(n=n, S=S, K=K, flags=0, step=1e-3, scan=8, N=N, max_flights=0, null=None, cat=None, D=0, cat_K=0):
        p = {k: (None if k == null else d(v)) for k, v in A.items()}
        q = {k: (None if cat is None or k == null else d(v)) for k, v in catalogue.items()}
        return lib.mpcx_collision_probability_mc(ctx, n, p["pairs"], S, K, None, p["Y"], None, p["units"], p["span"], p["consts"], flags, step, p["P0"], None,
                                                 None, p["radius"], D, cat_K, None, q["cat_Y"], q["cat_units"], q["cat_span"], q["cat_consts"], q["cat_P0"],
                                                 q["cat_radius"], p["half"], scan, N, 0, max_flights, None if null == "counts" else _ffi.lptr(counts),
                                                 p["out"], None if null == "status" else i(st), None, None, None)
    refused = [dict(n=0), dict(S=0), dict(K=1), dict(step=0.0), dict(step=-1.0), dict(flags=4), dict(flags=64), dict(flags=_ffi.FLAG_ATMO), dict(scan=0),
               dict(N=0), dict(max_flights=-1), dict(cat=True, D=0, cat_K=K), dict(cat=True, D=S, cat_K=1)] \
        + [dict(null=k) for k in list(A) + ["counts", "status"]] + [dict(cat=True, D=S, cat_K=K, null=k) for k in list(catalogue)[1:]]
    for bad in refused:
        assert call(**bad) == -2, bad
        assert b"collision_probability_mc" in lib.mpcx_last_error(ctx), (bad, lib.mpcx_last_error(ctx))
        assert (A["out"] == 7.0).all() and (counts == 7).all()
    w = lib.mpcx_collision_probability_mc_workspace_bytes
    assert w(0, 2, 5, 0, 0, 4, 0) == 0 and w(1, 2, 1, 0, 0, 4, 0) == 0 and w(1, 2, 5, 0, 0, 0, 0) == 0 and w(1, 2, 5, 1, 1, 4, 0) == 0
    assert w(1, 2, 5, 0, 0, 4, 0) >= 2 * 4 * 7 * 5 * 8 and w(1, 2, 5, 3, 9, 4, 0) > w(1, 2, 5, 0, 0, 4, 0) - 4 * 7 * 5 * 8
    assert w(1, 2, 5, 0, 0, 1 << 20, 64) < w(1, 2, 5, 0, 0, 1 << 20, 128) < w(1, 2, 5, 0, 0, 1 << 20, 0)
    assert lib.mpcx_collision_probability_mc_dev(ctx, n, None, S, K, *[None] * 6, 0, 1e-3, *[None] * 4, 0, 0, *[None] * 8, 8, N, 0, 0, *[None] * 8) == -2
    assert call() == 0 and (A["out"] != 7.0).all() and (counts != 7).all()     # (whatever the row's fate, the call runs and writes)


def test_constellation_mpc_collision_probability_mc():
    """test_collision_window_gpu.py's three-satellite plan with satellite 0 moved to pass 500 m from satellite 1: the method returns the
    screen, the window result on plan_covariance(P0, execution) and, bit for bit, the module-level Monte Carlo call on the plan"""
    from mpconstellation_amd import Satellite, ConstellationMPC, conjunction as cj
    from mpconstellation_amd.constellation import constellation_states
    from test_collision_window_gpu import result_bits
    st = constellation_states(3)
    mpc = ConstellationMPC([Satellite(s[:3].copy(), s[3:6].copy(), float(s[6])) for s in st], base_res=30, tf_horizon=2, tf_interval=1, r_des=1.5)
    mpc.update()
    (w,) = mpc._screen_windows("plan", samples_per_node=4)
    X = mpc._plan[0]
    m = w["M"] // 3
    tb = w["T0"] + m * ((w["T1"] - w["T0"]) / (w["M"] - 1))
    side = (X, w["units"], w["span"], np.zeros((3, X.shape[2], 6, 6)), np.zeros(3), w["ns"])
    _, pa, va, _, _ = C.state_and_cov_at(side, 0, tb, C.MU_EARTH)
    _, pb, vb, _, _ = C.state_and_cov_at(side, 1, tb, C.MU_EARTH)
    e = np.cross(vb - va, [0.0, 0.0, 1.0]); e /= np.linalg.norm(e)
    X[0, 0:3, :] += ((pb - pa + 500.0 * e) / w["units"][0, 0])[:, None]
    P0 = np.diag([100.0 ** 2] * 3 + [0.1 ** 2] * 3)
    ex = np.array([0.0, 0.02, 0.0, 0.01745, 0.0])
    scr, win, mc = mpc.collision_probability_mc(1000.0, P0, 50.0, 60.0, 256, seed=3, execution=ex, scan=32, return_samples=True)
    print("planted pair:", scr.pairs, "window p", win.p, "sampled", mc.p_hit, "+-", mc.se_hit, "counts", mc.counts.tolist())
    assert scr.pairs[:, :2].tolist() == [[0, 1]] and win.status.tolist() == [0] and mc.status.tolist() == [0] and mc.counts[0, 0] == 256
    P = cj.covariance_thrust(X, w["units"], w["span"], mpc.consts, P0, mpc._plan[1], ex, ns=w["ns"])
    win2 = cj.collision_probability_window(scr, 50.0, X, w["units"], w["span"], P, 60.0, panels=4, ns=w["ns"])
    mc2 = cj.collision_probability_mc(scr, 50.0, X, mpc._plan[1], w["units"], w["span"], mpc.consts, P0, 60.0, 256, seed=3, execution=ex, scan=32, ns=w["ns"],
                                      return_samples=True)
    assert result_bits(win) == result_bits(win2) and bits(mc) == bits(mc2) and np.array_equal(mc.samples, mc2.samples)
