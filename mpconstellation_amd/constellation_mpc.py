"""ConstellationMPC -- the reference's MPC loop for a whole constellation at once.

The reference runs OptimalController.update (control.py:166-235) for ONE satellite (`self.sats[0]`, :162) and
Simulator.run_segment calls it once per satellite in a Python loop (simulator.py:58-60).  Here every step of that loop
is one batched device call over all satellites, each with its own SatelliteScale (so each sees MU = 4 pi^2):

    reference rollout (tangential 0.5)  ->  SCPn x [ extract u_bar, discretise + solve, re-rollout under the
    optimised first-order-hold sequence over tf_u ]  ->  fly the segment under the truth model, update the states.

The number of nodes of the second SCP iteration is int(base_res * tf_u) and differs between satellites, as does the
length of the thrust table played back during the segment: those steps are ragged launches (include/mpcx.h,
mpcx_*_ragged: per-satellite node counts inside one rectangular batch), so each satellite gets exactly the result of the
single-satellite path (tests/test_mpc_loop_gpu.py) and the host never groups or loops over satellites."""
import time

import numpy as np

from . import _ffi
from .control import _check_solver_status
from .optimizer import mpc_step_batch, mpc_update_batch, scp_iteration_batch
from .satellite_scale import SatelliteScale
from .simulator import propagate_batch


def normalised_limits(scales, r_min=None, r_max=None, u_max=None, min_mass=None):
    """Physical limits -- radii in metres, thrust in newtons, mass in kilograms; scalars or one value per satellite -- as the
    options dict of a constellation whose satellites each live in their own units (SatelliteScale.units: length = the start radius,
    mass = the start mass, force derived from those): r_lim (S, 2), u_lim (S, 2) and min_mass (S,) in EACH satellite's units,
    ready for ConstellationMPC(options=...) and the batched calls of optimizer.py.  A common keep-out radius, engine or dry mass is
    then a different normalised number for every satellite.  Limits not given keep the defaults (optimizer.DEFAULT_OPTIONS)."""
    from .optimizer import DEFAULT_OPTIONS
    S = len(scales)
    unit = lambda name: np.array([sc.units[name] for sc in scales], dtype=np.float64)
    per_sat = lambda v: np.broadcast_to(np.asarray(v, dtype=np.float64), (S,))
    out = {}
    if r_min is not None or r_max is not None:
        lo = np.full(S, float(DEFAULT_OPTIONS["r_lim"][0])) if r_min is None else per_sat(r_min) / unit("length")
        hi = np.full(S, float(DEFAULT_OPTIONS["r_lim"][1])) if r_max is None else per_sat(r_max) / unit("length")
        out["r_lim"] = np.column_stack([lo, hi])
    if u_max is not None:
        out["u_lim"] = np.column_stack([np.full(S, float(DEFAULT_OPTIONS["u_lim"][0])), per_sat(u_max) / unit("force")])
    if min_mass is not None:
        out["min_mass"] = per_sat(min_mass) / unit("mass")
    return out


def _catalogue_keywords(trajectories):
    """a catalogue's trajectories (Y, units, span[, ns]) as the keywords conjunction's screens take; None: none"""
    return {} if trajectories is None else dict(zip(("cat_Y", "cat_units", "cat_span", "cat_ns"), trajectories))


class ConstellationMPC:
    def __init__(self, sats, base_res=100, tf_horizon=1, tf_interval=1, r_des=1.5, scp_iterations=2, sim_base_res=100,
                 include_drag=True, include_J2=True, device=0, strict=False, scales=None, verbose=False, devices=None,
                 time_parallel=False, plan_drag=False, plan_J2=False, options=None, atmosphere=None):
        self.sats = list(sats)
        # problem options on top of OPTIONS(horizon): the reference's keys, scalars or one value per satellite ((S,), (S, 2) for
        # u_lim / r_lim: _ffi.make_popts; normalised_limits above turns physical limits into them).  The user's values win.
        self.options = dict(options) if options else {}
        _ffi.make_popts(self.options, len(self.sats))      # (a wrong length is reported here, not at the first update)
        # every satellite in its own "designer units" (so that each sees MU = 4 pi^2) unless the caller brings the scales
        self.scales = list(scales) if scales is not None else [SatelliteScale(sat=s) for s in self.sats]
        self.verbose = verbose                # control.py:208-209's prints, per satellite
        self.consts = np.stack([sc.get_normalized_constants().as_vector() for sc in self.scales])
        self.base_res, self.sim_base_res = base_res, sim_base_res
        self.horizon, self.interval = tf_horizon, tf_interval
        self.r_des = np.broadcast_to(np.asarray(r_des, dtype=np.float64), (len(self.sats),)).copy()
        self.scp_iterations = scp_iterations
        self.include_drag, self.include_J2 = include_drag, include_J2          # the truth model the segments are flown with
        # the planning model: drag / J2 in every linearisation and every planning rollout (include/mpcx.h,
        # MPCX_FLAG_PLAN_ROLLOUTS), so that the plan predicts what a truth model with them flies.  Default: the reference's
        # planner, which has neither (control.py:187, 237-240)
        self.plan_drag, self.plan_J2 = bool(plan_drag), bool(plan_J2)
        # atmosphere (an Atmosphere): the altitude-dependent density (include/mpcx.h, MPCX_FLAG_ATMO) -- for the flown segments when
        # include_drag, for the plan when plan_drag; None: the reference's fixed density on both sides
        self.atmosphere = atmosphere
        self._plan_model = dict(include_drag=self.plan_drag, include_J2=self.plan_J2, rollout_model=self.plan_drag or self.plan_J2,
                                atmosphere=atmosphere)
        self.device = device
        # devices=[0, 1, ..., 7]: the constellation is dealt out in contiguous blocks to these devices, one host thread and one
        # context per device, no exchange between them (sharding.sharded_call) -- the reference loops over
        # its satellites serially (simulator.py:41,58)
        self.devices = list(devices) if devices is not None else None
        if verbose and self.devices is not None and len(self.devices) > 1:
            # (verbose prints control.py:208-209's lines between the SCP iterations: one library call per iteration on ONE
            #  context; silently solving on self.device while the flight is sharded would be neither of the two things asked for)
            raise ValueError("ConstellationMPC: verbose=True runs the SCP iterations as separate calls on one device; "
                             "use devices=[...] without verbose, or verbose with a single device")
        # time_parallel: the solves of small constellations (up to 128 satellites) on the time-parallel kernel (include/mpcx.h,
        # MPCX_SOLVE_TIME_PARALLEL: the horizon in four segments side by side; same iterations, not the other kernels' bits)
        self.solver_flags = _ffi.SOLVE_TIME_PARALLEL if time_parallel else 0
        self.strict = strict                  # raise instead of warning when a solve does not converge (control.py mirror)
        # per-satellite unit factors as vectors: the whole constellation is (re)dimensionalised in one array expression
        # (satellite_scale.py:46-100: r / r0, v / v0, m / m0 and back)
        self._f = np.array([[sc._r0, sc._v0, sc._m0] for sc in self.scales]).reshape(len(self.sats), 3)
        self._seg_y, self._seg_t, self._sim_cache = [], [], None       # flown segments (S,7,n) / (n,), and the dict view of them
        self._seg_tf = []                 # every flown segment's length in each satellite's own time unit (screen: its physical span)
        self.last_status = None           # (scp_iterations, S): every solve's MPCX_ST_* code of the last update
        self.last_iters = None            # ... and its interior-point iteration count
        self.plan_tf, self.plan_K = None, None
        self._plan = None                                               # (X, U, NU) of the last plan, rows of length Kmax
        self._plan_lists = None
        # wall-clock seconds spent inside the batched device calls (host staging included), accumulated over the updates
        self.timing = {"update": 0.0, "truth_propagation": 0.0}     # seconds inside the library calls (update [+ segment flight]; separate flight)

    def _timed(self, key, fn, *a, **kw):
        t0 = time.perf_counter()
        out = fn(*a, **kw)
        self.timing[key] += time.perf_counter() - t0
        return out

    def _y0(self):
        """normalised states of all satellites (SatelliteScale.normalize_state of each, in one expression)"""
        pos = np.array([s.position for s in self.sats], dtype=np.float64).reshape(-1, 3)
        vel = np.array([s.velocity for s in self.sats], dtype=np.float64).reshape(-1, 3)
        m = np.array([s.mass for s in self.sats], dtype=np.float64)
        f = self._f
        return np.column_stack([pos / f[:, 0:1], vel / f[:, 1:2], m / f[:, 2]])

    # the reference keeps sim_data / sim_time as dicts id -> array (simulator.py:18-19); built on demand from the batched
    # segments (one concatenation for the constellation instead of one per satellite and segment)
    def _sim_dicts(self):
        if self._sim_cache is None:
            if not self._seg_y:
                self._sim_cache = ({}, {})
            else:
                Y = np.concatenate(self._seg_y, axis=2); T = np.concatenate(self._seg_t)
                self._sim_cache = ({sat.id: Y[i] for i, sat in enumerate(self.sats)}, {sat.id: T.copy() for sat in self.sats})      # (an array per id, simulator.py:69-76)
        return self._sim_cache

    @property
    def sim_data(self):
        return self._sim_dicts()[0]

    @property
    def sim_time(self):
        return self._sim_dicts()[1]

    # the plan per satellite, trimmed to its own node count: lists of views, built on demand
    def _plan_views(self):
        if self._plan_lists is None and self._plan is not None:
            Kp = self.plan_K
            self._plan_lists = tuple([a[s][:, :Kp[s]] for s in range(len(self.sats))] for a in self._plan)
        return self._plan_lists or (None, None, None)

    @property
    def plan_x(self):
        return self._plan_views()[0]

    @property
    def plan_u(self):
        return self._plan_views()[1]

    @property
    def plan_nu(self):
        return self._plan_views()[2]

    # ---- OptimalController.update for every satellite ----
    OPTIONS = staticmethod(lambda horizon: {"eps_r": 0.000001, "eps_vr": 0.0000000000000001, "tf_max": horizon})      # control.py:192-197

    def update(self, y0=None, fly=None):
        """The whole update is ONE library call (mpc_update_batch -> mpcx_mpc_update_batch): reference rollout under the tangential
        controller (control.py:178-180), then per SCP iteration extract_uk, discretisation and solve, the re-rollout under the
        sequence just optimised sampled at int(base_res * tf_u) nodes per satellite (control.py:217-227, simulator.py:38: node
        counts computed on the device, ragged launches), the plan's thrust consumed in place -- only the final plan comes back.
        fly: also fly the segment (run_segment).  verbose=True prints control.py:208-209's lines per iteration and therefore runs
        the iterations as separate calls (scp_iteration_batch), with the same results bit for bit."""
        S = len(self.sats)
        y0 = self._y0() if y0 is None else y0
        K = int(self.base_res * self.horizon)
        opts = {**self.OPTIONS(self.horizon), **self.options}
        for flags in ((self.solver_flags, 0) if self.solver_flags & _ffi.SOLVE_TIME_PARALLEL else (self.solver_flags,)):
            if self.verbose:
                res = self._update_by_iterations(y0, K, opts, flags)
                flown = None
            else:
                res = self._timed("update", mpc_update_batch, y0, float(self.horizon), self.consts, self.r_des, self.base_res,
                                  n_scp=self.scp_iterations, options=opts, device=self.device, fly=fly, devices=self.devices,
                                  flags=flags, **self._plan_model)
                self._check(res.prop_status)
                self.last_status = res.status; self.last_iters = res.iters
                flown = (res.y_sim, res.sim_status) if fly is not None else None
            # A time-parallel solve whose workgroups could not all run at once (the device shared with another long kernel:
            # MPCX_ST_TIMEOUT, include/mpcx.h) is not a failed plan: the update is done again on the default kernels.
            if flags & _ffi.SOLVE_TIME_PARALLEL and (np.asarray(self.last_status) == 10).any():
                import warnings
                warnings.warn("time-parallel solve timed out waiting for its workgroups (device busy?): update repeated on the default kernels",
                              RuntimeWarning, stacklevel=2)
                continue
            break
        for it in range(self.scp_iterations):
            _check_solver_status(np.asarray(self.last_status)[it], self.strict)
        self.plan_K = res.Ks.astype(np.int32)
        self._plan = (res.X, res.U, res.NU)                                # rows of length K; U is the table the segment is flown with
        self._plan_lists = None
        self.plan_tf = res.tf.copy()
        if self.horizon - self.interval > 0.1:                               # control.py:234-235
            self.horizon -= self.interval
        return flown

    def _update_by_iterations(self, y0, K, opts, flags=0):
        """the same update as one library call per SCP iteration (the plan crosses PCIe between them): what verbose mode needs"""
        S = len(self.sats)
        tf_u = np.full(S, float(self.horizon))
        law = (_ffi.CTRL_TANGENTIAL, np.array([0.5]), 0, None)
        Ks = None; Kus = None                                              # first iteration: K nodes for everybody
        self.last_status = np.zeros((self.scp_iterations, S), dtype=np.int32); self.last_iters = np.zeros_like(self.last_status)
        res = None
        for it in range(self.scp_iterations):
            res = self._timed("update", scp_iteration_batch, y0, tf_u, self.consts, self.r_des, law, K, options=opts,
                              Ks=Ks, Kus=Kus, device=self.device, flags=flags, **self._plan_model)
            self._check(res.prop_status)
            self.last_status[it] = res.status; self.last_iters[it] = res.iters
            for j in range(S):
                print(f"tf for optimizer: {res.tf[j]}")
                print(f"Total virtual control effort: {np.abs(res.NU[j]).sum()}")
            tf_u = res.tf.copy()
            if it == self.scp_iterations - 1:
                break                 # (the reference re-rolls once more, control.py:227, and drops the result)
            Kus = Ks                                                       # columns in use of the table the next rollout plays
            Ks = (self.base_res * res.tf).astype(np.int32)                 # ... sampled at int(base_res * tf_u) nodes
            law = (_ffi.CTRL_SEQUENCE, res.U, K, 1.0)                      # SequenceController(u_opt, tf_u, tf_sim = tf_u)
        res.Ks = np.full(S, K, dtype=np.int32) if Ks is None else Ks
        return res

    # ---- Simulator.run_segment for every satellite: plan, fly tf under the truth model, update the states ----
    def run_segment(self, tf=1):
        y0 = self._y0()
        n_eval = int(self.sim_base_res * tf)
        # SequenceController(tf_u, tf_sim = interval): end_tau = tf_u / interval; the flight rides in the update's call
        flown = self.update(y0, fly=(tf, self.interval, n_eval, self.include_drag, self.include_J2, 0.001))
        y, st = self._fly_stored_plan(y0, tf, n_eval) if flown is None else flown      # (verbose path: the flight as its own call)
        self._segment_flown(y, st, tf, n_eval)

    def fly_plan(self, tf=1):
        """Fly tf under the truth model with the plan the instance HOLDS (the last update's, or one put in its place), without
        planning again: run_segment without its update -- the same playback of the thrust table (SequenceController(tf_u,
        tf_sim = interval)), the same bookkeeping (the satellites' states, the flown segment), and the horizon is left alone."""
        if self._plan is None:
            raise ValueError("fly_plan: the instance holds no plan yet (update or run_segment)")
        n_eval = int(self.sim_base_res * tf)
        y, st = self._fly_stored_plan(self._y0(), tf, n_eval)
        self._segment_flown(y, st, tf, n_eval)

    def _fly_stored_plan(self, y0, tf, n_eval):
        """the stored plan's thrust table played back from y0 over tf under the truth model -> (y, status)"""
        U = self._plan[1]
        y, st, _ = self._timed("truth_propagation", propagate_batch, y0, tf, self.consts,
                               (_ffi.CTRL_SEQUENCE, U, U.shape[2], self.plan_tf / self.interval), n_eval,
                               self.include_drag, self.include_J2, 0.001, self.device, Kus=self.plan_K, devices=self.devices,
                               atmosphere=self.atmosphere)
        return y, st

    def _segment_flown(self, y, st, tf, n_eval):
        """run_segment's tail: check the flight, move the satellites to its end, keep the segment"""
        self._check(st)
        t = np.linspace(0, 1, n_eval)
        f = self._f
        end = np.column_stack([y[:, 0:3, -1] * f[:, 0:1], y[:, 3:6, -1] * f[:, 1:2], y[:, 6, -1] * f[:, 2]])     # redim_state
        for i, sat in enumerate(self.sats):
            sat.update_state_vector(end[i])
        if self._seg_t:
            t = t + self._seg_t[-1][-1] * tf + 0.0000001                  # simulator.py:69-76
        self._seg_y.append(y); self._seg_t.append(t); self._seg_tf.append(float(tf)); self._sim_cache = None

    def run_segments(self, tf=1, num_segments=1):
        for _ in range(num_segments):
            self.run_segment(tf=tf / float(num_segments))

    # ---- conjunction screening: all satellites on one clock (conjunction.py) ----
    def _screen_windows(self, what="flown", samples_per_node=4, T0=None, T1=None):
        """What `screen` hands to conjunction.screen, one dict per window -- Y, ns, units, span, M, T0, T1: every satellite's
        units are its scale's length and time unit; a flown segment q spans (sum of the earlier segments' tf, that sum + its own
        tf) times the satellite's time unit, a plan (0, plan_tf) times it with plan_K nodes in use.  [T0, T1], unless given, is the
        intersection of the satellites' spans; the grid has samples_per_node intervals per node interval of the longest row."""
        if int(samples_per_node) != samples_per_node or samples_per_node < 1:
            raise ValueError(f"samples_per_node: need an integer >= 1, got {samples_per_node}")
        units = np.array([[sc.units["length"], sc.units["time"]] for sc in self.scales], dtype=np.float64)
        if what == "flown":
            if not self._seg_y:
                raise ValueError("screen(what='flown'): no segment has been flown yet (run_segment)")
            t_end = np.cumsum(self._seg_tf)
            rows = [(y, None, np.outer(units[:, 1], [t1 - tf, t1])) for y, tf, t1 in zip(self._seg_y, self._seg_tf, t_end)]
        elif what == "plan":
            if self._plan is None:
                raise ValueError("screen(what='plan'): there is no plan yet (update)")
            rows = [(self._plan[0], np.asarray(self.plan_K, dtype=np.int32),
                     np.column_stack([np.zeros(len(self.sats)), np.asarray(self.plan_tf) * units[:, 1]]))]
        else:
            raise ValueError(f"screen: what = {what!r}, expected 'flown' or 'plan'")
        out = []
        for Y, ns, span in rows:
            t0 = float(span[:, 0].max()) if T0 is None else float(T0)
            t1 = float(span[:, 1].min()) if T1 is None else float(T1)
            if not t1 > t0:
                raise ValueError(f"screen: the satellites' spans have no common interval ([{t0}, {t1}] s)")
            n = Y.shape[2] if ns is None else int(ns.max())
            out.append(dict(Y=Y, ns=ns, units=units, span=span, M=int(samples_per_node) * (max(n, 2) - 1) + 1, T0=t0, T1=t1))
        return out

    def screen(self, threshold_m, samples_per_node=4, what="flown", T0=None, T1=None, max_pairs=None):
        """Closest approaches inside the constellation (conjunction.screen; distances in metres, times in seconds since the start
        of the first flown segment, or of the plan): what='flown' screens every flown segment on its own common grid and combines
        them (conjunction.combine); what='plan' the last plan.  Returns a ConjunctionResult: dmin, partner, tca per satellite and
        the pairs at or below threshold_m."""
        from . import conjunction as cj
        kw = {} if max_pairs is None else {"max_pairs": max_pairs}
        res = [cj.screen(threshold=threshold_m, device=self.device, devices=self.devices, **w, **kw)
               for w in self._screen_windows(what, samples_per_node, T0, T1)]
        return res[0] if len(res) == 1 else cj.combine(res)

    def screen_against(self, catalogue, threshold_m, samples_per_node=4, what="flown", T0=None, T1=None, max_pairs=None):
        """Closest approaches of the constellation to a catalogue of foreign objects (conjunction.screen_against).  catalogue =
        (Y, units, span) or (Y, units, span, ns): the objects' trajectories in their own units, span in the seconds of `screen`'s
        times (since the start of the first flown segment, or of the plan).  The windows are `screen`'s: the constellation's spans
        alone decide T0 and T1; an object outside its span there is NaN and is ignored.  Flown windows are combined
        (conjunction.combine).  Returns a ConjunctionResult: dmin, partner (a catalogue index), tca per satellite and the pairs
        (satellite, object) at or below threshold_m; status and cat_status are the ephemerides' when there is one window (a plan,
        one flown segment) and None when several were combined."""
        from . import conjunction as cj
        if len(catalogue) not in (3, 4):
            raise ValueError(f"catalogue: expected (Y, units, span) or (Y, units, span, ns), got {len(catalogue)} items")
        kw = {} if max_pairs is None else {"max_pairs": max_pairs}
        res = [cj.screen_against(threshold=threshold_m, device=self.device, devices=self.devices, **w, **_catalogue_keywords(catalogue), **kw)
               for w in self._screen_windows(what, samples_per_node, T0, T1)]
        return res[0] if len(res) == 1 else cj.combine(res)

    def plan_covariance(self, P0, q=None, execution=None, mass_var0=None, density=None):
        """The covariance (S, plan_K, 6, 6) of the last plan at its nodes under the planning model's flags and atmosphere (plan_drag,
        plan_J2): conjunction.covariance along (plan X, plan U, plan_tf, plan_K) from P0 with the acceleration noise q when execution
        is None, otherwise conjunction.covariance_thrust with the thrust execution errors execution ((5,) or (S, 5):
        conjunction.gates_execution) and the mass variance mass_var0 at the first node.  density ((2,) or (S, 2) = (sigma, tau in
        seconds; np.inf: a bias)): conjunction.covariance_drag, the same with an uncertain drag (execution and mass_var0 optional);
        it needs plan_drag=True -- without drag the planning model has no density to be uncertain about."""
        (w,) = self._screen_windows("plan", 1)                            # (the plan's nodes, units and span: the grid is not used)
        return self._plan_covariance(w, P0, q, execution, mass_var0, density)

    def _plan_covariance(self, w, P0, q, execution, mass_var0, density=None):
        from . import conjunction as cj
        where = dict(device=self.device, devices=self.devices)
        if density is not None:
            if not self.plan_drag:
                raise ValueError("density: the planning model has no drag (plan_drag=False), so there is no density to be uncertain about")
            model = self._conjunction_model()
            return cj.covariance_drag(w["Y"], w["units"], w["span"], self.consts, P0, density, U=self._plan[1], execution=execution,
                                      mass_var0=mass_var0, ns=w["ns"], q=q, include_J2=model["include_J2"], atmosphere=model["atmosphere"], **where)
        if execution is None:
            if mass_var0 is not None:
                raise ValueError("mass_var0: a mass variance needs execution (covariance carries no mass)")
            return cj.covariance(w["Y"], w["units"], w["span"], self.consts, P0, U=self._plan[1], ns=w["ns"], q=q, **self._conjunction_model(),
                                 **where)
        return cj.covariance_thrust(w["Y"], w["units"], w["span"], self.consts, P0, self._plan[1], execution, mass_var0=mass_var0, ns=w["ns"],
                                    q=q, **self._conjunction_model(), **where)

    def _conjunction_model(self, model="plan"):
        """the model keywords of conjunction's linearising calls: 'plan' the planning model (plan_drag, plan_J2), 'truth' the model the
        segments are flown with (include_drag, include_J2); the atmosphere beside the drag"""
        if model not in ("plan", "truth"):
            raise ValueError(f"model: expected 'plan' or 'truth', got {model!r}")
        drag, J2 = (self.plan_drag, self.plan_J2) if model == "plan" else (self.include_drag, self.include_J2)
        return dict(include_drag=drag, include_J2=J2, atmosphere=self.atmosphere if drag else None)

    def _u_max(self):
        """every satellite's thrust limit: the upper bound of this instance's u_lim option, per-satellite tables included"""
        from .optimizer import DEFAULT_OPTIONS
        u_lim = np.asarray({**DEFAULT_OPTIONS, **self.OPTIONS(self.horizon), **self.options}["u_lim"], dtype=np.float64)
        return np.ascontiguousarray(np.broadcast_to(u_lim[..., 1], (len(self.sats),)))

    @staticmethod
    def _catalogue_with_radii(catalogue):
        """catalogue = (Y, units, span, P, radius[, ns]) -> (what conjunction's probabilities take as cat, its trajectories (Y, units, span,
        ns) for the screen); None: (None, None)"""
        if catalogue is None:
            return None, None
        if len(catalogue) not in (5, 6):
            raise ValueError(f"catalogue: expected (Y, units, span, P, radius) or (Y, units, span, P, radius, ns), got {len(catalogue)} items")
        cat = tuple(catalogue)
        return cat, cat[:3] + (cat[5] if len(cat) == 6 else None,)

    @staticmethod
    def _catalogue_plain(catalogue):
        """catalogue = (Y, units, span[, P][, ns]) -> (what conjunction's avoidance calls take as cat, its trajectories (Y, units, span, ns)
        for the screen); None: (None, None)"""
        if catalogue is None:
            return None, None
        if not 3 <= len(catalogue) <= 5:
            raise ValueError(f"catalogue: expected (Y, units, span[, P][, ns]), got {len(catalogue)} items")
        cat = tuple(catalogue)
        counts = [a for a in cat[3:] if a is None or np.ndim(a) != 4]      # (what follows the span and is not P)
        ns = counts[0] if counts else None
        return cat, cat[:3] + (None if ns is None else np.ascontiguousarray(ns, dtype=np.int32),)

    def _screen_plan(self, threshold_m, samples_per_node, max_pairs, trajectories=None):
        """the last plan's screen window, its pairs list at threshold_m -- inside the constellation, or against the catalogue whose
        trajectories = (Y, units, span, ns) are given -- and the device keywords -> (w, screened, where)"""
        from . import conjunction as cj
        (w,) = self._screen_windows("plan", samples_per_node)
        kw = {} if max_pairs is None else {"max_pairs": max_pairs}
        where = dict(device=self.device, devices=self.devices)
        screen = cj.screen if trajectories is None else cj.screen_against
        return w, screen(threshold=threshold_m, **_catalogue_keywords(trajectories), **where, **w, **kw), where

    def _plan_probabilities(self, threshold_m, P0, q, samples_per_node, max_pairs, catalogue, execution=None, mass_var0=None, density=None):
        """what the probabilities and the window manoeuvres start from: the plan screened at threshold_m (against catalogue = (Y, units,
        span, P, radius[, ns]) if given) and its covariance -> (w, screened, P, the keywords ns, cat, device and devices)"""
        if density is not None and not self.plan_drag:                   # (refused before anything is screened)
            raise ValueError("density: the planning model has no drag (plan_drag=False), so there is no density to be uncertain about")
        cat, trajectories = self._catalogue_with_radii(catalogue)
        w, screened, where = self._screen_plan(threshold_m, samples_per_node, max_pairs, trajectories)
        return w, screened, self._plan_covariance(w, P0, q, execution, mass_var0, density), dict(ns=w["ns"], cat=cat, **where)

    @staticmethod
    def _window_choice(half_window, max_half, nsigma):
        """half_window of the window methods, tested before anything is screened: a number or one per listed pair (False; max_half
        belongs to 'auto' and is refused), or the string 'auto' (True) with max_half None, a positive finite scalar or an array of
        them, and a positive finite nsigma"""
        if not isinstance(half_window, str):
            if max_half is not None:
                raise ValueError("max_half: goes with half_window='auto'; a given half_window is used as it is")
            return False
        if half_window != "auto":
            raise ValueError(f"half_window: expected seconds (a scalar or one per listed pair) or 'auto', got {half_window!r}")
        if max_half is not None:
            mh = np.asarray(max_half)
            if mh.ndim > 1 or mh.dtype.kind not in "iuf" or not (np.isfinite(mh).all() and (mh > 0.0).all()):
                raise ValueError(f"max_half: need positive finite seconds (a scalar or one per listed pair) or None, got {max_half!r}")
        if np.ndim(nsigma) != 0 or isinstance(nsigma, str) or not (nsigma > 0.0 and np.isfinite(nsigma)):
            raise ValueError(f"nsigma: need a positive finite number, got {nsigma!r}")
        return True

    def _chosen_window(self, auto, half_window, max_half, nsigma, w, screened, radius_m, P, plan):
        """-> (the half_window the window calls receive, what the method's tuple gains): the given one and nothing; with 'auto' the
        .half of conjunction.encounter_window on the screened rows, the plan and its covariance -- max_half None: half the plan's
        common span -- and that EncounterWindowResult"""
        if not auto:
            return half_window, ()
        from . import conjunction as cj
        if max_half is None:
            max_half = 0.5 * (w["T1"] - w["T0"])
        chosen = cj.encounter_window(screened, radius_m, w["Y"], w["units"], w["span"], P, max_half, nsigma=nsigma, **plan)
        return chosen.half, (chosen,)

    def collision_probability(self, threshold_m, P0, radius_m, q=None, samples_per_node=4, max_pairs=None, catalogue=None, execution=None,
                              mass_var0=None, density=None):
        """Collision probabilities of the last plan's close approaches -> (ConjunctionResult, CollisionResult).  The plan is screened
        at threshold_m (screen(what='plan'); screen_against when catalogue = (Y, units, span, P, radius) or (Y, units, span, P,
        radius, ns) is given: the objects' trajectories, their covariances -- conjunction.catalogue_covariance -- and hard-body
        radii); P0 ((6, 6) or (S, 6, 6); m, m/s), the covariance of every satellite at the plan's first node, is propagated along
        (plan X, plan U, plan_tf, plan_K) under the planning model's flags and atmosphere (plan_drag, plan_J2) with the acceleration
        noise q (plan_covariance: conjunction.covariance, or with execution / mass_var0 conjunction.covariance_thrust, the covariance
        with thrust execution errors, or with density conjunction.covariance_drag, the covariance with an uncertain drag), and
        every listed pair gets its probability (conjunction.collision_probability; radius_m a scalar or (S,)).  The plan only: a
        linearisation needs the thrust a trajectory was flown with, and ConstellationMPC does not keep the thrust of its flown
        segments."""
        from . import conjunction as cj
        w, screened, P, plan = self._plan_probabilities(threshold_m, P0, q, samples_per_node, max_pairs, catalogue, execution, mass_var0, density)
        return screened, cj.collision_probability(screened, radius_m, w["Y"], w["units"], w["span"], P, **plan)

    def collision_probability_window(self, threshold_m, P0, radius_m, half_window, panels=4, q=None, samples_per_node=4, max_pairs=None,
                                     catalogue=None, execution=None, mass_var0=None, *, max_half=None, nsigma=8, density=None):
        """collision_probability and the window probability of the same rows -> (ConjunctionResult, CollisionResult,
        WindowCollisionResult).  The screening arguments, P0, radius_m, q, catalogue, execution, mass_var0 and density are
        collision_probability's, and the first two results are what it returns; every listed pair also gets its probability over
        [t - half_window, t + half_window] (conjunction.collision_probability_window on the same plan, covariances and radii;
        half_window a scalar or one per listed pair, in seconds; panels as there).  For the pairs of a constellation that pass each other slowly the short-encounter figure
        is outside its model, and without relative speed it fails: the window figure is the one to read there.  half_window='auto':
        every listed pair's window is chosen on the device (conjunction.encounter_window on the same rows, plan, covariances and radii,
        searching max_half seconds to either side -- a scalar or one per listed pair; None: half the plan's common span -- for the
        stretch within nsigma combined sigmas of a collision), its .half is what the window call receives, and the
        EncounterWindowResult is returned as a fourth element.  The plan only."""
        from . import conjunction as cj
        auto = self._window_choice(half_window, max_half, nsigma)
        w, screened, P, plan = self._plan_probabilities(threshold_m, P0, q, samples_per_node, max_pairs, catalogue, execution, mass_var0, density)
        half_window, chosen = self._chosen_window(auto, half_window, max_half, nsigma, w, screened, radius_m, P, plan)
        return (screened, cj.collision_probability(screened, radius_m, w["Y"], w["units"], w["span"], P, **plan),
                cj.collision_probability_window(screened, radius_m, w["Y"], w["units"], w["span"], P, half_window, panels=panels, **plan)) + chosen

    def collision_probability_mc(self, threshold_m, P0, radius_m, half_window, samples, seed=0, execution=None, mass_var0=None, scan=64,
                                 panels=4, model="plan", samples_per_node=4, max_pairs=None, prop_max_step=1e-3, max_flights=0,
                                 return_samples=False, return_trajectories=False, *, max_half=None, nsigma=8):
        """The window probability of the last plan's close approaches and its Monte Carlo counterpart side by side ->
        (ConjunctionResult, WindowCollisionResult, MonteCarloCollisionResult).  The plan is screened at threshold_m inside the
        constellation; the window figure is conjunction.collision_probability_window on plan_covariance(P0, execution=execution,
        mass_var0=mass_var0) -- no acceleration noise: the samples have none --; the sampled figure is
        conjunction.collision_probability_mc on the same rows, plan, P0, execution errors and radii: `samples` worlds drawn with
        `seed` and flown under model = 'plan' (plan_drag, plan_J2, what the covariance was linearised under) or 'truth' (the model the
        segments are flown with).  half_window='auto' with max_half and nsigma as in collision_probability_window: both figures run
        over the chosen windows and the EncounterWindowResult is a fourth element.  The plan only."""
        from . import conjunction as cj
        auto = self._window_choice(half_window, max_half, nsigma)
        w, screened, P, plan = self._plan_probabilities(threshold_m, P0, None, samples_per_node, max_pairs, None, execution, mass_var0)
        plan.pop("cat")
        half_window, chosen = self._chosen_window(auto, half_window, max_half, nsigma, w, screened, radius_m, P, plan)
        return (screened, cj.collision_probability_window(screened, radius_m, w["Y"], w["units"], w["span"], P, half_window, panels=panels, **plan),
                cj.collision_probability_mc(screened, radius_m, w["Y"], self._plan[1], w["units"], w["span"], self.consts, P0, half_window, samples,
                                            seed=seed, scan=scan, execution=execution, mass_var0=mass_var0, prop_max_step=prop_max_step,
                                            max_flights=max_flights, return_samples=return_samples, return_trajectories=return_trajectories,
                                            **self._conjunction_model(model), **plan)) + chosen

    def avoidance_window(self, threshold_m, P0, radius_m, half_window, target_p, panels=4, q=None, samples_per_node=4, max_pairs=None,
                         catalogue=None, who="i", tol=_ffi.AW_DEFAULT_TOL, max_eval=_ffi.AW_DEFAULT_MAX_EVAL, *, max_half=None, nsigma=8):
        """Avoidance for the last plan's slow close approaches -> (ConjunctionResult, WindowCollisionResult, AvoidanceWindowResult).
        The plan is screened and its covariance propagated exactly as collision_probability_window does (the same arguments);
        every listed pair gets its window probability and the thrust change of conjunction.avoidance_window on (plan X, plan U,
        plan_tf, plan_K) under the planning model's flags and atmosphere that brings that probability down to target_p; who = 'i',
        'j' or 'both' (inside the constellation) says which satellite of a pair moves.  AvoidanceWindowResult.apply(plan U, row) is
        the changed thrust table.  The covariances are not propagated again under the manoeuvre and nothing is flown
        (avoidance_window_refine does both).  half_window='auto' with max_half and nsigma as in collision_probability_window: the
        probability and the manoeuvre run over the chosen windows and the EncounterWindowResult is a fourth element.  The plan only."""
        from . import conjunction as cj
        auto = self._window_choice(half_window, max_half, nsigma)
        w, screened, P, plan = self._plan_probabilities(threshold_m, P0, q, samples_per_node, max_pairs, catalogue)
        half_window, chosen = self._chosen_window(auto, half_window, max_half, nsigma, w, screened, radius_m, P, plan)
        return (screened, cj.collision_probability_window(screened, radius_m, w["Y"], w["units"], w["span"], P, half_window, panels=panels, **plan),
                cj.avoidance_window(screened, target_p, radius_m, w["Y"], self._plan[1], w["units"], w["span"], self.consts, P, half_window,
                                    panels=panels, who=who, tol=tol, max_eval=max_eval, **self._conjunction_model(), **plan)) + chosen

    def avoidance_window_refine(self, threshold_m, P0, radius_m, half_window, target_p, rounds=2, model="plan", recov=True, panels=4, q=None,
                                samples_per_node=4, max_pairs=None, catalogue=None, who="i", track=True, max_shift=None,
                                tol=_ffi.AW_DEFAULT_TOL, max_eval=_ffi.AW_DEFAULT_MAX_EVAL, prop_max_step=1e-3, *, max_half=None, nsigma=8):
        """avoidance_window's manoeuvres flown again, re-evaluated and corrected `rounds` times on the device -> (ConjunctionResult,
        WindowCollisionResult, AvoidanceWindowRefineResult).  The plan is screened and its covariance propagated exactly as
        avoidance_window does (the same arguments); every listed pair then goes through conjunction.avoidance_window_refine on (plan X,
        plan U, plan_tf, plan_K): its time is tracked on the plan's screen window (samples_per_node; track=False holds it on the given
        time), with recov the covariances of the satellites that move are propagated again along every flight with the same q.  model
        = 'plan' flies and linearises under the planning model (plan_drag, plan_J2), 'truth' under the model the segments are flown
        with (include_drag, include_J2, the atmosphere).  Nothing is installed: the manoeuvres are row-private, and two rows that move
        one satellite can conflict (AvoidanceWindowRefineResult.apply(plan U, row) is one row's changed thrust table).
        half_window='auto' with max_half and nsigma as in collision_probability_window: the windows are chosen once, on the plan as it
        stands (they do not follow the manoeuvre from pass to pass), and the EncounterWindowResult is a fourth element.  The plan
        only."""
        from . import conjunction as cj
        auto = self._window_choice(half_window, max_half, nsigma)
        flight = self._conjunction_model(model)
        w, screened, P, plan = self._plan_probabilities(threshold_m, P0, q, samples_per_node, max_pairs, catalogue)
        half_window, chosen = self._chosen_window(auto, half_window, max_half, nsigma, w, screened, radius_m, P, plan)
        return (screened, cj.collision_probability_window(screened, radius_m, w["Y"], w["units"], w["span"], P, half_window, panels=panels, **plan),
                cj.avoidance_window_refine(screened, target_p, radius_m, w["Y"], self._plan[1], w["units"], w["span"], self.consts, P, half_window,
                                           rounds=rounds, track=(w["M"], w["T0"], w["T1"]) if track else None, max_shift=max_shift, recov=recov,
                                           q=q, prop_max_step=prop_max_step, panels=panels, who=who, tol=tol, max_eval=max_eval, **flight, **plan)) + chosen

    def _screened_plan(self, threshold_m, samples_per_node, max_pairs, catalogue, P0, q):
        """what `avoidance` and `avoidance_joint` start from: the plan's screen window, its pairs list at threshold_m (inside the
        constellation, or against catalogue = (Y, units, span[, P][, ns])), the plan's covariance when P0 is given, the catalogue as
        a tuple and as the screens' keywords, and the device keywords -> (w, screened, P, cat, cat_kw, where)"""
        cat, trajectories = self._catalogue_plain(catalogue)
        w, screened, where = self._screen_plan(threshold_m, samples_per_node, max_pairs, trajectories)
        return w, screened, None if P0 is None else self._plan_covariance(w, P0, q, None, None), cat, _catalogue_keywords(trajectories), where

    def encounters(self, threshold_m, P0=None, radius_m=None, q=None, samples_per_node=4, max_pairs=None, max_events=16, catalogue=None):
        """EVERY close approach of the last plan's listed pairs, not only the closest -> (ConjunctionResult, EncounterEvents).  The
        plan is screened at threshold_m as `avoidance` screens it (screen(what='plan'); screen_against with a catalogue), and
        conjunction.screen_events returns every encounter of the listed pairs at or below the same threshold, at most max_events
        per pair: a plan of several revolutions holds about two per revolution for crossing orbits.  With P0 ((6, 6) or (S, 6, 6);
        m, m/s) and radius_m (a scalar or (S,)) it returns (ConjunctionResult, EncounterEvents, CollisionResult, cumulative): the
        plan's covariance is propagated as collision_probability propagates it, every event gets its own probability
        (conjunction.collision_probability over events.events) and every listed pair the probability of at least one collision
        over its events (conjunction.cumulative_probability, (n,)).  catalogue = (Y, units, span) or (Y, units, span, ns) for the
        events alone; (Y, units, span, P, radius) or (Y, units, span, P, radius, ns) with P0 and radius_m, as collision_probability
        takes it.  The plan only, as there."""
        from . import conjunction as cj
        if (P0 is None) != (radius_m is None):
            raise ValueError("P0 and radius_m come together (probabilities) or not at all (the events alone)")
        cat, cat_kw, trajectories = None, {}, None
        if catalogue is not None:
            cat = tuple(catalogue)
            if len(cat) not in ((5, 6) if P0 is not None else (3, 4)):
                raise ValueError("catalogue: expected (Y, units, span, P, radius[, ns]) with P0 and radius_m, (Y, units, span[, ns]) "
                                 f"without, got {len(cat)} items")
            cat_ns = cat[-1] if len(cat) in (4, 6) else None
            trajectories = cat[:3] if cat_ns is None else cat[:3] + (cat_ns,)
            cat_kw = dict(cat_Y=cat[0], cat_units=cat[1], cat_span=cat[2], cat_ns=cat_ns)
        w, screened, P, _, _, where = self._screened_plan(threshold_m, samples_per_node, max_pairs, trajectories, P0, q)
        events = cj.screen_events(screened, threshold=threshold_m, max_events=max_events, **w, **cat_kw, **where)
        if P0 is None:
            return screened, events
        col = cj.collision_probability(events.events, radius_m, w["Y"], w["units"], w["span"], P, ns=w["ns"], cat=cat, **where)
        return screened, events, col, cj.cumulative_probability(events, col.pc)

    def avoidance(self, threshold_m, target, P0=None, q=None, samples_per_node=4, max_pairs=None, catalogue=None, who="i"):
        """Avoidance manoeuvres for the last plan's close approaches -> (ConjunctionResult, AvoidanceResult).  The plan is screened
        at threshold_m as collision_probability screens it (screen(what='plan'); screen_against when catalogue = (Y, units, span),
        (Y, units, span, P) or (Y, units, span, P, ns) is given); with P0 ((6, 6) or (S, 6, 6); m, m/s) the satellites' covariance
        is propagated along the plan with the acceleration noise q and `target` is a Mahalanobis distance (a catalogue then needs
        its P), without it `target` is a miss distance in metres; every listed pair gets the least-effort thrust change of
        conjunction.avoidance on (plan X, plan U, plan_tf, plan_K) under the planning model's flags and atmosphere; who = 'i', 'j'
        or 'both' (inside the constellation) says which satellite of a pair moves.  AvoidanceResult.apply(plan U, row) is the changed
        thrust table; feeding it back into the solver's constraints is not done here."""
        from . import conjunction as cj
        w, screened, P, cat, _, where = self._screened_plan(threshold_m, samples_per_node, max_pairs, catalogue, P0, q)
        return screened, cj.avoidance(screened, target, w["Y"], self._plan[1], w["units"], w["span"], self.consts, ns=w["ns"], P=P, cat=cat,
                                      who=who, **self._conjunction_model(), **where)

    def avoidance_joint(self, threshold_m, target, P0=None, q=None, samples_per_node=4, max_pairs=None, catalogue=None, who="i",
                        hold_terminal=True, tol=_ffi.AJ_DEFAULT_TOL, max_iter=_ffi.AJ_DEFAULT_MAX_ITER, return_rows=False,
                        return_terminal=False):
        """One manoeuvre per satellite for ALL of the last plan's close approaches it moves for -> (ConjunctionResult,
        AvoidanceJointResult).  The plan is screened and, with P0, its covariance propagated exactly as `avoidance` does; every
        manoeuvring satellite then gets the thrust change of conjunction.avoidance_joint on (plan X, plan U, plan_tf, plan_K) under
        the planning model: all of its encounters opened to `target` at once, inside its own thrust limit -- the upper bound of
        this instance's u_lim option, per-satellite tables included -- and, with hold_terminal, the plan's last position and
        velocity held to first order.  who = 'i' or 'j'; an (n,) array of 0 / 1 only for a caller who has screened the same plan at
        the same threshold before (screen(what='plan') / screen_against) and so knows the list.  AvoidanceJointResult.apply(plan U)
        is the changed thrust table; the solver-side encounter rows remain open, this call is their check."""
        from . import conjunction as cj
        w, screened, P, cat, _, where = self._screened_plan(threshold_m, samples_per_node, max_pairs, catalogue, P0, q)
        return screened, cj.avoidance_joint(screened, target, w["Y"], self._plan[1], w["units"], w["span"], self.consts, ns=w["ns"], P=P,
                                            cat=cat, who=who, u_max=self._u_max(), hold_terminal=hold_terminal, tol=tol, max_iter=max_iter,
                                            return_rows=return_rows, return_terminal=return_terminal, **self._conjunction_model(), **where)

    def avoidance_refine(self, threshold_m, target, rounds=3, P0=None, q=None, samples_per_node=4, max_pairs=None, catalogue=None, who="i",
                         hold_terminal=True, tol=_ffi.AJ_DEFAULT_TOL, max_iter=_ffi.AJ_DEFAULT_MAX_ITER, prop_max_step=1e-3, model="plan",
                         install=False, return_rows=False, return_terminal=False, return_rhs=False, events=False, max_events=16):
        """avoidance_joint's manoeuvre flown again, re-screened and corrected `rounds` times on the device -> (ConjunctionResult,
        AvoidanceRefineResult).  The plan is screened as avoidance_joint screens it, u_max comes from this instance's u_lim option,
        the re-screen's grid and span are the plan's screen window (samples_per_node).  model = 'plan' flies and linearises under the
        planning model (plan_drag, plan_J2), 'truth' under the model the segments are flown with (include_drag, include_J2, the
        atmosphere).  install=True puts Y_flown and U + du of every satellite whose status is 0 into the plan the instance holds, so
        that fly_plan flies the refined manoeuvre.
        events=True: EVERY close approach of the listed pairs at or below threshold_m is opened, not only each pair's closest -- the
        list is conjunction.screen_events' (at most max_events per pair, as `encounters` lists them), every row follows its own
        encounter through the re-screens (conjunction.avoidance_refine(track=True)), and the return is (ConjunctionResult,
        EncounterEvents, AvoidanceRefineResult) with the result's rows in events.events' order.  A satellite that moves for more
        than MPCX_AJ_MAX_ROWS = 8 rows gets MPCX_ST_BADK = 9 as from avoidance_joint; who as an array has one entry per event then."""
        from . import conjunction as cj
        flight = self._conjunction_model(model)
        w, screened, P, cat, cat_kw, where = self._screened_plan(threshold_m, samples_per_node, max_pairs, catalogue, P0, q)
        found = cj.screen_events(screened, threshold=threshold_m, max_events=max_events, **w, **cat_kw, **where) if events else None
        res = cj.avoidance_refine(screened if found is None else found.events, target, w["Y"], self._plan[1], w["units"], w["span"], self.consts,
                                  w["M"], w["T0"], w["T1"], track=found is not None,
                                  rounds=rounds, ns=w["ns"], P=P, cat=cat, who=who, u_max=self._u_max(), hold_terminal=hold_terminal, tol=tol,
                                  max_iter=max_iter, prop_max_step=prop_max_step, return_rows=return_rows, return_terminal=return_terminal,
                                  return_rhs=return_rhs, device=self.device, devices=None if self.devices is None else list(self.devices)[:1],
                                  **flight)
        if install:
            ok = (res.status == 0) & np.isfinite(res.du).all(axis=(1, 2))
            X, U = np.array(self._plan[0], dtype=np.float64), np.array(self._plan[1], dtype=np.float64)
            X[ok] = res.Y_flown[ok]
            U[ok] = U[ok] + res.du[ok]
            self._plan = (X, U) + tuple(self._plan[2:])
        return (screened, res) if found is None else (screened, found, res)

    @staticmethod
    def _check(status):
        if (status == 1).any():
            raise Exception("ERROR: INVALID SATELLITE MASS")               # simulator.py:135-136
        if (status != 0).any():
            raise RuntimeError(f"propagation failed: {[_ffi.STATUS_TEXT.get(int(c), c) for c in status if c]}")
