"""ctypes binding of libmpcx.so (include/mpcx.h).  No CPU fallback: if the HIP library or a
gfx950 device is missing, every compute entry point raises."""
import ctypes as C
import os
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MPCX_LIB") or os.path.join(HERE, "libmpcx.so")      # (MPCX_LIB: another build of the same library, for A/B measurements)

STATUS_TEXT = {
    0: "ok", 1: "satellite mass <= 0", 2: "RK45 step size underflow",
    3: "FOH index outside the input table", 4: "state-transition matrix singular",
    5: "solver hit max_iter", 6: "solver numeric breakdown", 7: "solver stopped at acceptable level",
    9: "ragged batch: node / table-column / output-point count outside the accepted range",
    8: "constraint set empty (start node outside its radius bounds, terminal window outside r_max, empty window or tf range)",
    10: "time-parallel solve: a workgroup of the satellite did not answer within the wait limit (device shared with another long kernel?)",
}
FLAG_DRAG, FLAG_J2, FLAG_UNIFORM_STEPS, FLAG_RK23, FLAG_PLAN_ROLLOUTS, FLAG_ATMO = 1, 2, 4, 8, 16, 32
FLAG_DRAG_COLUMN = 64      # mpcx_discretize_stages*_dev with FLAG_DRAG: the drag column G_k in the record's Sigma slot
NATMO = 4
CTRL_ZERO, CTRL_CONSTANT, CTRL_TANGENTIAL, CTRL_SEQUENCE = 0, 1, 2, 3
NCONST = 8
STAGE_DOUBLES = 105
NTERM_SCALARS = 8

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_lp = C.POINTER(C.c_int64)
_vp = C.c_void_p


class MpcxError(RuntimeError):
    pass


_lib = None
_lock = threading.Lock()
_ctxs = {}

class SolveOpts(C.Structure):
    """mpcx_solve_opts (include/mpcx.h)"""
    _fields_ = [(n, C.c_double) for n in ("min_mass", "u_max", "r_min", "r_max", "eps_r", "eps_vr", "eps_vn", "eps_vt",
                                          "tf_max", "w_nu", "w_tr", "tol", "acceptable_tol")] + \
               [(n, C.c_int32) for n in ("max_iter", "acceptable_iter", "n_refine", "flags")]


_po = C.POINTER(SolveOpts)

_SIGS = {
    "mpcx_version": (C.c_int, []),
    "mpcx_create": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "mpcx_destroy": (None, [_vp]),
    "mpcx_last_error": (C.c_char_p, [_vp]),
    "mpcx_synchronize": (C.c_int, [_vp, _vp]),
    "mpcx_set_stream": (C.c_int, [_vp, _vp]),
    "mpcx_set_atmosphere": (C.c_int, [_vp, _dp]),
    "mpcx_trace_enable": (C.c_int, [_vp, C.c_int]),
    "mpcx_last_call_trace": (C.c_int, [_vp, _dp, C.c_int]),
    "mpcx_host_alloc": (_vp, [_vp, C.c_size_t]),
    "mpcx_host_free": (None, [_vp, _vp]),
    "mpcx_discretize_batch": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.c_int,
                                        C.c_double, _dp, _dp, _dp, _dp, _dp, _ip]),
    "mpcx_discretize_batch_dev": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp,
                                            C.c_int, C.c_double, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mpcx_discretize_stages_dev": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp,
                                             C.c_int, C.c_double, _vp, _vp, _vp]),
    "mpcx_propagate_batch": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, _dp, C.c_int, C.c_int, _dp, C.c_int, _dp,
                                       C.c_double, _dp, _ip, _ip]),
    "mpcx_propagate_batch_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, _vp, C.c_int, _vp,
                                           C.c_double, _vp, _vp, _vp, _vp]),
    "mpcx_default_solve_opts": (None, [_po]),
    "mpcx_solve_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "mpcx_mpc_step_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "mpcx_solve_workspace_bytes_ctx": (C.c_size_t, [_vp, C.c_int, C.c_int]),
    "mpcx_mpc_step_workspace_bytes_ctx": (C.c_size_t, [_vp, C.c_int, C.c_int]),
    "mpcx_solve_batch": (C.c_int, [_vp, C.c_int, C.c_int] + [_dp] * 10 + [_po, _dp, _dp, _dp, _dp, _ip, _ip, _dp]),
    "mpcx_solve_regularised": (C.c_int, [_vp, C.c_int, _ip]),
    "mpcx_solve_regularised_dev": (C.c_int, [_vp, C.c_int, _vp, _vp]),
    "mpcx_constraint_terms": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, _dp, _po, _dp, _dp, _dp]),
    "mpcx_constraint_terms_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, _po, _vp, _vp, _vp, _vp]),
    "mpcx_solve_batch_dev": (C.c_int, [_vp, C.c_int, C.c_int] + [_vp] * 6 + [_po] + [_vp] * 7 + [_vp, _vp]),
    "mpcx_mpc_step_batch": (C.c_int, [_vp, C.c_int, C.c_int] + [_dp] * 5 + [C.c_int, C.c_double, _po, _dp, _dp, _dp, _dp,
                                                                         _ip, _ip, _dp]),
    "mpcx_mpc_step_batch_dev": (C.c_int, [_vp, C.c_int, C.c_int] + [_vp] * 5 + [C.c_int, C.c_double, _po] + [_vp] * 7
                                + [_vp, _vp]),
    # ragged batches (per-satellite node counts)
    "mpcx_discretize_stages_ragged_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp,
                                                    C.c_int, C.c_double, _vp, _vp, _vp]),
    "mpcx_solve_batch_ragged_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp] + [_vp] * 6 + [_po] + [_vp] * 7 + [_vp, _vp]),
    "mpcx_mpc_step_batch_ragged": (C.c_int, [_vp, C.c_int, C.c_int, _ip] + [_dp] * 5 + [C.c_int, C.c_double, _po, _dp, _dp, _dp,
                                                                                     _dp, _ip, _ip, _dp]),
    "mpcx_mpc_step_batch_ragged_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp] + [_vp] * 5 + [C.c_int, C.c_double, _po] + [_vp] * 7
                                       + [_vp, _vp]),
    "mpcx_propagate_batch_ragged": (C.c_int, [_vp, C.c_int, C.c_int, _ip, _dp, _dp, _dp, C.c_int, C.c_int, _dp, C.c_int, _ip,
                                              _dp, C.c_double, _dp, _ip, _ip]),
    "mpcx_propagate_batch_ragged_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, C.c_int, C.c_int, _vp, C.c_int,
                                                  _vp, _vp, C.c_double, _vp, _vp, _vp, _vp]),
    "mpcx_propagate_thrust_batch_ragged": (C.c_int, [_vp, C.c_int, C.c_int, _ip, _dp, _dp, _dp, C.c_int, C.c_int, _dp, C.c_int, _ip,
                                                     _dp, C.c_double, _dp, _dp, _ip, _ip]),
    "mpcx_propagate_thrust_batch_ragged_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, C.c_int, C.c_int, _vp, C.c_int,
                                                         _vp, _vp, C.c_double, _vp, _vp, _vp, _vp, _vp]),
    "mpcx_scp_iteration_batch_ragged": (C.c_int, [_vp, C.c_int, C.c_int, _ip, _dp, _dp, _dp, _dp, C.c_int, C.c_int, _dp, C.c_int, _ip, _dp,
                                                  C.c_double, C.c_int, C.c_double, _po, _dp, _dp, _dp, _dp, _dp, _dp, _ip, _ip, _dp, _ip]),
    "mpcx_mpc_update_batch": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_double, _dp, _dp, _dp, _dp, C.c_double, C.c_double, C.c_int,
                                        C.c_double, _po, _dp, _dp, _dp, _dp, _ip, _ip, _ip, _dp, _ip, C.c_double, C.c_double, C.c_int, C.c_int,
                                        C.c_double, _dp, _ip]),
    "mpcx_resample_sequence_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp]),
    # conjunction screening (the constellation on one clock, all-pairs closest approach)
    "mpcx_ephemeris_batch": (C.c_int, [_vp, C.c_int, C.c_int, _ip, _dp, _dp, _dp, C.c_int, C.c_double, C.c_double, _dp, _ip]),
    "mpcx_ephemeris_batch_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, C.c_int, C.c_double, C.c_double, _vp, _vp, _vp]),
    "mpcx_conjunction_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "mpcx_conjunction_screen": (C.c_int, [_vp, C.c_int, C.c_int, _dp, C.c_double, C.c_double, C.c_int, C.c_int, C.c_double, C.c_int,
                                          _dp, _ip, _dp, _dp, _lp]),
    "mpcx_conjunction_screen_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_double, C.c_double, C.c_int, C.c_int, C.c_double, C.c_int,
                                              _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mpcx_conjunction_screen_traj": (C.c_int, [_vp, C.c_int, C.c_int, _ip, _dp, _dp, _dp, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int,
                                               C.c_double, C.c_int, _dp, _ip, _dp, _dp, _lp, _ip]),
    # the constellation against a catalogue of foreign objects (rows x columns instead of the union's square)
    "mpcx_conjunction_cross_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "mpcx_conjunction_cross_screen": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _dp, _dp, C.c_double, C.c_double, C.c_int, C.c_int, C.c_double,
                                                C.c_int, _dp, _ip, _dp, _dp, _lp]),
    "mpcx_conjunction_cross_screen_dev": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_double, C.c_double, C.c_int, C.c_int,
                                                    C.c_double, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mpcx_conjunction_cross_screen_traj": (C.c_int, [_vp, C.c_int, C.c_int, _ip, _dp, _dp, _dp, C.c_int, C.c_int, _ip, _dp, _dp, _dp, C.c_int,
                                                     C.c_double, C.c_double, C.c_int, C.c_int, C.c_double, C.c_int, _dp, _ip, _dp, _dp, _lp,
                                                     _ip, _ip]),
    # the closest approach of listed pairs alone (a screen's list looked at again on changed trajectories)
    "mpcx_conjunction_pairs_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "mpcx_conjunction_pairs": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, C.c_int, _dp, _dp, C.c_double, C.c_double, _dp, _ip]),
    "mpcx_conjunction_pairs_dev": (C.c_int, [_vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_double, C.c_double, _vp, _vp, _vp]),
    "mpcx_conjunction_pairs_traj": (C.c_int, [_vp, C.c_int, _dp] + [C.c_int, C.c_int, _ip, _dp, _dp, _dp] * 2
                                    + [C.c_int, C.c_double, C.c_double, _dp, _ip, _ip, _ip]),
    "mpcx_conjunction_pairs_traj_dev": (C.c_int, [_vp, C.c_int, _vp] + [C.c_int, C.c_int, _vp, _vp, _vp, _vp] * 2
                                        + [C.c_int, C.c_double, C.c_double, _vp, _vp, _vp, _vp, _vp, _vp]),
    # every close approach of listed pairs below a threshold (the pairs calls with threshold, max_events and four outputs)
    "mpcx_conjunction_events_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "mpcx_conjunction_events": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, C.c_int, _dp, _dp, C.c_double, C.c_double, C.c_double, C.c_int,
                                          _dp, _ip, _ip, _ip]),
    "mpcx_conjunction_events_dev": (C.c_int, [_vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_double, C.c_double, C.c_double,
                                              C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "mpcx_conjunction_events_traj": (C.c_int, [_vp, C.c_int, _dp] + [C.c_int, C.c_int, _ip, _dp, _dp, _dp] * 2
                                     + [C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, _dp, _ip, _ip, _ip, _ip, _ip]),
    "mpcx_conjunction_events_traj_dev": (C.c_int, [_vp, C.c_int, _vp] + [C.c_int, C.c_int, _vp, _vp, _vp, _vp] * 2
                                         + [C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    # the close approach nearest each listed row's own time (the pairs calls with max_shift and an optional info output)
    "mpcx_conjunction_track_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "mpcx_conjunction_track": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, C.c_int, _dp, _dp, C.c_double, C.c_double, C.c_double, _dp, _ip, _ip]),
    "mpcx_conjunction_track_dev": (C.c_int, [_vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_double, C.c_double, C.c_double, _vp, _vp,
                                             _vp, _vp]),
    "mpcx_conjunction_track_traj": (C.c_int, [_vp, C.c_int, _dp] + [C.c_int, C.c_int, _ip, _dp, _dp, _dp] * 2
                                    + [C.c_int, C.c_double, C.c_double, C.c_double, _dp, _ip, _ip, _ip, _ip]),
    "mpcx_conjunction_track_traj_dev": (C.c_int, [_vp, C.c_int, _vp] + [C.c_int, C.c_int, _vp, _vp, _vp, _vp] * 2
                                        + [C.c_int, C.c_double, C.c_double, C.c_double, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    # collision probability of screened pairs: covariance along trajectories, then the encounter-plane integral per listed pair
    "mpcx_covariance_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "mpcx_covariance_batch": (C.c_int, [_vp, C.c_int, C.c_int, _ip, _dp, _dp, _dp, _dp, _dp, C.c_int, C.c_double, _dp, _dp, _dp, _ip]),
    "mpcx_covariance_batch_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_double, _vp, _vp, _vp, _vp,
                                            _vp, _vp]),
    # the same chain over all seven states with thrust execution errors (after q: exec, m_var0; after P: Pm)
    "mpcx_covariance_thrust_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "mpcx_covariance_thrust_batch": (C.c_int, [_vp, C.c_int, C.c_int, _ip, _dp, _dp, _dp, _dp, _dp, C.c_int, C.c_double, _dp, _dp, _dp, _dp,
                                               _dp, _dp, _ip]),
    "mpcx_covariance_thrust_batch_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_double, _vp, _vp, _vp,
                                                   _vp, _vp, _vp, _vp, _vp, _vp]),
    # the chain over eight states with an uncertain drag (after m_var0: dens; after Pm: Pb)
    "mpcx_covariance_drag_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "mpcx_covariance_drag_batch": (C.c_int, [_vp, C.c_int, C.c_int, _ip, _dp, _dp, _dp, _dp, _dp, C.c_int, C.c_double, _dp, _dp, _dp, _dp,
                                             _dp, _dp, _dp, _dp, _ip]),
    "mpcx_covariance_drag_batch_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_double, _vp, _vp, _vp,
                                                 _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mpcx_collision_probability": (C.c_int, [_vp, C.c_int, _dp] + [C.c_int, C.c_int, _ip, _dp, _dp, _dp, _dp, _dp] * 2 + [C.c_double, _dp, _ip]),
    "mpcx_collision_probability_dev": (C.c_int, [_vp, C.c_int, _vp] + [C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp] * 2
                                       + [C.c_double, _vp, _vp, _vp]),
    # the same list over a time window: the ball at its start plus the expected entries, from the full 6 x 6 covariances
    "mpcx_collision_probability_window": (C.c_int, [_vp, C.c_int, _dp] + [C.c_int, C.c_int, _ip, _dp, _dp, _dp, _dp, _dp] * 2
                                          + [C.c_double, _dp, C.c_int, _dp, _ip]),
    "mpcx_collision_probability_window_dev": (C.c_int, [_vp, C.c_int, _vp] + [C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp] * 2
                                              + [C.c_double, _vp, C.c_int, _vp, _vp, _vp]),
    # the time window of every listed row, chosen on the device (after mu: max_half, nsigma, levels; out, flags, status)
    "mpcx_encounter_window": (C.c_int, [_vp, C.c_int, _dp] + [C.c_int, C.c_int, _ip, _dp, _dp, _dp, _dp, _dp] * 2
                              + [C.c_double, _dp, C.c_double, C.c_int, _dp, _ip, _ip]),
    "mpcx_encounter_window_dev": (C.c_int, [_vp, C.c_int, _vp] + [C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp] * 2
                                  + [C.c_double, _vp, C.c_double, C.c_int, _vp, _vp, _vp, _vp]),
    # avoidance manoeuvres for screened pairs: thrust sensitivities of the encounter-plane miss, least-effort thrust change
    "mpcx_avoidance_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "mpcx_avoidance": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, _ip, _dp, _dp, _dp, _dp, _dp, C.c_int, C.c_double, _dp,
                                 C.c_int, C.c_int, _ip, _dp, _dp, _dp, _dp, C.c_double, C.c_double, C.c_int, _dp, _dp, _dp, _ip]),
    "mpcx_avoidance_dev": (C.c_int, [_vp, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_double, _vp,
                                     C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_double, C.c_double, C.c_int, _vp, _vp, _vp, _vp,
                                     _vp, _vp]),
    # avoidance for slow encounters: the window probability's derivative with respect to the thrust nodes, a target on that probability
    "mpcx_collision_window_sensitivity_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "mpcx_collision_window_sensitivity": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, _ip, _dp, _dp, _dp, _dp, _dp, C.c_int, C.c_double,
                                                    _dp, _dp, C.c_int, C.c_int, _ip, _dp, _dp, _dp, _dp, _dp, C.c_double, _dp, C.c_int,
                                                    C.c_int, _dp, _dp, _dp, _ip]),
    "mpcx_collision_window_sensitivity_dev": (C.c_int, [_vp, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int,
                                                        C.c_double, _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_double,
                                                        _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mpcx_avoidance_window_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "mpcx_avoidance_window": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, _ip, _dp, _dp, _dp, _dp, _dp, C.c_int, C.c_double, _dp, _dp,
                                        C.c_int, C.c_int, _ip, _dp, _dp, _dp, _dp, _dp, C.c_double, _dp, C.c_int, C.c_int, C.c_double,
                                        C.c_double, C.c_int, _dp, _dp, _dp, _ip]),
    "mpcx_avoidance_window_dev": (C.c_int, [_vp, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_double, _vp, _vp,
                                            C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_double, _vp, C.c_int, C.c_int, C.c_double,
                                            C.c_double, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp]),
    # the window manoeuvre flown, re-evaluated and corrected, a fixed number of rounds on the device (after max_eval: prop_max_step,
    # rounds, M, T0, T1, max_shift, recov, q)
    "mpcx_avoidance_window_refine_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "mpcx_avoidance_window_refine": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, _ip, _dp, _dp, _dp, _dp, _dp, C.c_int, C.c_double, _dp,
                                               _dp, C.c_int, C.c_int, _ip, _dp, _dp, _dp, _dp, _dp, C.c_double, _dp, C.c_int, C.c_int,
                                               C.c_double, C.c_double, C.c_int, C.c_double, C.c_int, C.c_int, C.c_double, C.c_double,
                                               C.c_double, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip, _dp, _dp, _dp, _dp, _dp]),
    "mpcx_avoidance_window_refine_dev": (C.c_int, [_vp, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_double,
                                                   _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_double, _vp, C.c_int,
                                                   C.c_int, C.c_double, C.c_double, C.c_int, C.c_double, C.c_int, C.c_int, C.c_double,
                                                   C.c_double, C.c_double, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                                   _vp, _vp]),
    # joint avoidance: all of a satellite's encounters under its thrust limit, one small convex problem per manoeuvring satellite
    "mpcx_avoidance_joint_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "mpcx_avoidance_joint": (C.c_int, [_vp, C.c_int, _dp, _ip, C.c_int, C.c_int, _ip, _dp, _dp, _dp, _dp, _dp, C.c_int, C.c_double, _dp,
                                       C.c_int, C.c_int, _ip, _dp, _dp, _dp, _dp, C.c_double, C.c_double, _dp, C.c_int, C.c_double, C.c_int,
                                       C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _ip, _ip]),
    "mpcx_avoidance_joint_dev": (C.c_int, [_vp, C.c_int, _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_double, _vp,
                                           C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_double, C.c_double, _vp, C.c_int, C.c_double,
                                           C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    # iterated avoidance: the joint manoeuvre flown again, re-screened and corrected, a fixed number of rounds on the device
    "mpcx_avoidance_refine_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "mpcx_avoidance_refine": (C.c_int, [_vp, C.c_int, _dp, _ip, C.c_int, C.c_int, _ip, _dp, _dp, _dp, _dp, _dp, C.c_int, C.c_double, _dp,
                                        C.c_int, C.c_int, _ip, _dp, _dp, _dp, _dp, C.c_double, C.c_double, _dp, C.c_int, C.c_double, C.c_int,
                                        C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, _dp, _dp, _dp, _dp, _dp, _ip, _ip,
                                        _dp, _dp, _dp, _dp, _dp, _ip, _dp, _dp]),
    "mpcx_avoidance_refine_dev": (C.c_int, [_vp, C.c_int, _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_double, _vp,
                                            C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_double, C.c_double, _vp, C.c_int, C.c_double,
                                            C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp,
                                            _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    # the same loop with the re-screen that follows each row's own encounter (max_shift after rounds)
    "mpcx_avoidance_refine_tracked": (C.c_int, [_vp, C.c_int, _dp, _ip, C.c_int, C.c_int, _ip, _dp, _dp, _dp, _dp, _dp, C.c_int, C.c_double, _dp,
                                                C.c_int, C.c_int, _ip, _dp, _dp, _dp, _dp, C.c_double, C.c_double, _dp, C.c_int, C.c_double, C.c_int,
                                                C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_double, _dp, _dp, _dp, _dp, _dp, _ip, _ip,
                                                _dp, _dp, _dp, _dp, _dp, _ip, _dp, _dp]),
    "mpcx_avoidance_refine_tracked_dev": (C.c_int, [_vp, C.c_int, _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_double, _vp,
                                                    C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_double, C.c_double, _vp, C.c_int, C.c_double,
                                                    C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_double, _vp, _vp, _vp, _vp,
                                                    _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    # the collision probability by sampled flights through the truth model (after flags: prop_max_step, P0, exec, m_var0, radius; the
    # catalogue with its consts; half_window, scan, n_samples, seed, max_flights; counts, out, status, samples, Y_samples, U_samples)
    "mpcx_collision_probability_mc_workspace_bytes": (C.c_size_t, [C.c_int] * 7),
    "mpcx_collision_probability_mc": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, _ip, _dp, _dp, _dp, _dp, _dp, C.c_int, C.c_double, _dp,
                                                _dp, _dp, _dp, C.c_int, C.c_int, _ip, _dp, _dp, _dp, _dp, _dp, _dp, _dp, C.c_int, C.c_int,
                                                C.c_uint64, C.c_int, _lp, _dp, _ip, _dp, _dp, _dp]),
    "mpcx_collision_probability_mc_dev": (C.c_int, [_vp, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_double,
                                                    _vp, _vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int,
                                                    C.c_int, C.c_uint64, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
}
NMCC, NMC, NMS = 6, 9, 5                                                    # MPCX_NMCC, MPCX_NMC, MPCX_NMS: columns of mpcx_collision_probability_mc's counts, out, samples
MCC_FLOWN, MCC_FAILED, MCC_START, MCC_ENTRIES, MCC_SQUARES, MCC_HIT = range(NMCC)
MC_P_HIT, MC_SE_HIT, MC_START, MC_ENTRIES, MC_SE_BOUND, MC_EXCESS, MC_TA, MC_TB, MC_N_OK = range(NMC)
MS_DMIN, MS_T_MIN, MS_INSIDE_START, MS_ENTRIES, MS_STATUS = range(NMS)
NDENS = 2                                                                  # MPCX_NDENS: (sigma_b, tau_b) of mpcx_covariance_drag_batch's dens
NEXEC = 5                                                                  # MPCX_NEXEC: (s_fm, s_pm, s_fp, s_pp, u_off) of mpcx_covariance_thrust_batch's exec
NPC = 6                                                                     # MPCX_NPC: columns of mpcx_collision_probability's out
PC_P, PC_MISS, PC_SPEED, PC_SIGMA1, PC_SIGMA2, PC_MAHAL = range(NPC)
NPW, PW_MAX_PANELS = 7, 64                                                  # MPCX_NPW: columns of mpcx_collision_probability_window's out
PW_P, PW_START, PW_ENTRIES, PW_RATE_MAX, PW_T_RATE_MAX, PW_TA, PW_TB = range(NPW)
NEW, EW_MAX_LEVELS = 6, 4                                                   # MPCX_NEW: columns of mpcx_encounter_window's out
EW_HALF, EW_TA, EW_TB, EW_REACH_BEFORE, EW_REACH_AFTER, EW_G0 = range(NEW)
EW_CLEAR, EW_OPEN_BEFORE, EW_OPEN_AFTER, EW_BAD_SCAN = 1, 2, 4, 8           # MPCX_EW_*: bits of its flags
NAV = 10                                                                    # MPCX_NAV: columns of mpcx_avoidance's out
AV_D0, AV_D1, AV_DM1, AV_DM2, AV_MISS1, AV_DT, AV_DV_I, AV_DV_J, AV_UMAX_I, AV_UMAX_J = range(NAV)
NAW = 9                                                                     # MPCX_NAW: columns of mpcx_avoidance_window's out
AW_P0, AW_P1, AW_ALPHA, AW_DQ_LINEAR, AW_DV_I, AW_DV_J, AW_UMAX_I, AW_UMAX_J, AW_EVALS = range(NAW)
AW_DEFAULT_TOL, AW_DEFAULT_MAX_EVAL = 1e-6, 40
NAJ, NAR, AJ_MAX_ROWS = 8, 5, 8                                             # MPCX_NAJ, MPCX_NAR: columns of mpcx_avoidance_joint's sat_out, row_out
AJ_COST, AJ_DV, AJ_UMAX, AJ_ROWS, AJ_ACTIVE, AJ_ONBALL, AJ_ITERS, AJ_RESIDUAL = range(NAJ)
AR_D0, AR_MARGIN, AR_DIST, AR_LAMBDA, AR_DT = range(NAR)
AJ_DEFAULT_TOL, AJ_DEFAULT_MAX_ITER = 1e-10, 50


def _sat_twin(name):
    """(name, signature) of an entry point's per-satellite twin (include/mpcx.h): `_sat` in the name, the option table
    popts [S][NPOPT] directly after the options pointer"""
    res, args = _SIGS[name]
    dev = name.endswith("_dev")
    i = args.index(_po) + 1
    return (name[:-4] + "_sat_dev" if dev else name + "_sat"), (res, args[:i] + [_vp if dev else _dp] + args[i:])


_SIGS.update([_sat_twin(n) for n in ("mpcx_constraint_terms", "mpcx_constraint_terms_dev", "mpcx_solve_batch", "mpcx_solve_batch_ragged_dev",
                                     "mpcx_mpc_step_batch_ragged", "mpcx_mpc_step_batch_ragged_dev", "mpcx_scp_iteration_batch_ragged",
                                     "mpcx_mpc_update_batch")])


def exported_symbols():
    return list(_SIGS)


def load():
    """dlopen libmpcx.so and declare signatures.  Raises MpcxError if it is not built."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise MpcxError(f"{LIB_PATH} is missing: run `python -m mpconstellation_amd.build` "
                                "(hipcc, gfx950). There is no CPU fallback.")
            lib = C.CDLL(LIB_PATH)
            for name, (res, args) in _SIGS.items():
                fn = getattr(lib, name)
                fn.restype = res
                fn.argtypes = args
            _lib = lib
    return _lib


def context(device=0, slot=0):
    """One mpcx context per (process, device, slot).  Calls on different contexts are thread-safe and run on their own
    streams (include/mpcx.h): host threads that want to overlap small launches take different slots."""
    lib = load()
    device = (device, slot) if slot else device
    with _lock:
        if device not in _ctxs:
            h = _vp()
            rc = lib.mpcx_create(device[0] if isinstance(device, tuple) else device, C.byref(h))
            if rc != 0:
                raise MpcxError(f"mpcx_create(device={device}) failed ({rc}): "
                                f"{lib.mpcx_last_error(None).decode()}")
            _ctxs[device] = h
        return _ctxs[device]


STREAM_PRIVATE = C.c_void_p(-1)


def set_stream(stream, device=0, slot=0):
    """Run the host-pointer entry points of this context on `stream` (a hipStream_t as an integer, e.g.
    torch.cuda.current_stream().cuda_stream; None / 0: the device's default stream; STREAM_PRIVATE: a private stream again).
    For processes that also drive the device through another stream: include/mpcx.h, mpcx_set_stream."""
    lib = load(); ctx = context(device, slot)
    check(lib.mpcx_set_stream(ctx, stream if isinstance(stream, C.c_void_p) else C.c_void_p(stream or 0)), ctx, "mpcx_set_stream")


def set_atmosphere(ctx, atmosphere):
    """mpcx_set_atmosphere: give context `ctx` the atmosphere that its calls with FLAG_ATMO use -- an Atmosphere
    (mpconstellation_amd.atmosphere), anything with coefficients(), or the four numbers (c0, c1, c2, h_floor); None clears it."""
    if atmosphere is None:
        check(load().mpcx_set_atmosphere(ctx, None), ctx, "mpcx_set_atmosphere")
        return
    coef = as_f64(atmosphere.coefficients() if hasattr(atmosphere, "coefficients") else atmosphere)
    if coef.shape != (NATMO,):
        raise ValueError(f"atmosphere: expected {NATMO} coefficients (c0, c1, c2, h_floor), got shape {coef.shape}")
    check(load().mpcx_set_atmosphere(ctx, dptr(coef)), ctx, "mpcx_set_atmosphere")


def atmosphere_context(device=0, slot=0, atmosphere=None):
    """context(device, slot), given `atmosphere` first when there is one: what a wrapper whose flags carry FLAG_ATMO calls on.
    A call without an atmosphere leaves the context's alone (its flags do not carry the bit, so it is not read)."""
    ctx = context(device, slot)
    if atmosphere is not None:
        set_atmosphere(ctx, atmosphere)
    return ctx


TRACE_FIELDS = ("wall_ms", "first_marker_ms", "host_stage_ms", "host_wait_ms", "host_copyout_ms", "dev_span_ms", "dev_kernels_ms", "valid")


def trace_enable(on=True, device=0, slot=0):
    """every following host-pointer call of this context records where its time went (include/mpcx.h, mpcx_trace_enable)"""
    lib = load(); ctx = context(device, slot)
    check(lib.mpcx_trace_enable(ctx, 1 if on else 0), ctx, "mpcx_trace_enable")


def last_call_trace(device=0, slot=0):
    """the record of the context's last traced host-pointer call as a dict (TRACE_FIELDS), or None if there is none"""
    lib = load(); ctx = context(device, slot)
    out = np.zeros(len(TRACE_FIELDS))
    check(lib.mpcx_last_call_trace(ctx, dptr(out), len(out)), ctx, "mpcx_last_call_trace")
    return dict(zip(TRACE_FIELDS, out.tolist())) if out[-1] else None


class _PinnedOwner:
    """keeps a page-locked allocation alive as long as a numpy array views it"""

    def __init__(self, ctx, ptr, nbytes):
        self.ctx, self.ptr = ctx, ptr
        self.buf = (C.c_char * nbytes).from_address(ptr)

    def __del__(self):
        try:
            load().mpcx_host_free(self.ctx, self.ptr)
        except Exception:
            pass


def pinned_empty(shape, dtype=np.float64, device=0):
    """numpy array in page-locked host memory (mpcx_host_alloc): the host-pointer entry points transfer such arrays by DMA
    without a staging copy.  Use it for arrays handed to mpc_step_batch / solve_batch repeatedly."""
    lib = load(); ctx = context(device)
    dt = np.dtype(dtype)
    n = int(np.prod(shape)) * dt.itemsize
    ptr = lib.mpcx_host_alloc(ctx, max(n, 1))
    if not ptr:
        raise MpcxError(f"mpcx_host_alloc({n}) failed: {lib.mpcx_last_error(ctx).decode()}")
    owner = _PinnedOwner(ctx, ptr, max(n, 1))
    owner.buf._mpcx_owner = owner            # the array keeps buf alive, buf keeps the allocation's owner alive
    arr = np.frombuffer(owner.buf, dtype=dt, count=int(np.prod(shape))).reshape(shape)
    return arr


def pinned_copy(a, device=0):
    a = np.asarray(a)
    out = pinned_empty(a.shape, a.dtype, device)
    out[...] = a
    return out


class _ResultPool:
    """Result arrays of the batched wrappers, recycled.  A large numpy array is a fresh anonymous mapping: the first write to
    each of its pages is a page fault, and for the 17 MB a 4096-satellite step returns those faults are 1.8 ms of a 8.8 ms call on
    average and 3-5 ms now and then -- every call, because numpy unmaps the arrays of the previous results
    when the caller drops them.  take() hands out an array of the pool when NOBODY else holds a reference to it any more (the
    previous results have been dropped: reference count of the pooled object = the pool's own) and a new one otherwise, so a
    caller that keeps its results keeps them untouched.  A few arrays per shape, a few shapes."""
    PER_SHAPE, SHAPES = 3, 24

    def __init__(self):
        self._lock = threading.Lock()
        self._pool = {}          # (shape, dtype) -> [arrays]

    def take(self, shape, dtype=np.float64):
        import sys
        key = (tuple(int(n) for n in shape), np.dtype(dtype).str)
        nbytes = int(np.prod(key[0])) * np.dtype(dtype).itemsize
        if nbytes < (1 << 20):                                   # small arrays come from malloc's own free lists: nothing to gain
            return np.empty(shape, dtype=dtype)
        with self._lock:
            lst = self._pool.get(key)
            if lst is None:
                if len(self._pool) >= self.SHAPES:
                    self._pool.pop(next(iter(self._pool)))
                lst = self._pool[key] = []
            else:
                self._pool[key] = self._pool.pop(key)            # (most recently used last)
            for i in range(len(lst)):
                if sys.getrefcount(lst[i]) == 2:                 # the list's reference and getrefcount's argument: nobody else
                    return lst[i]
            a = np.empty(shape, dtype=dtype)
            if len(lst) < self.PER_SHAPE:
                lst.append(a)
            return a


result_pool = _ResultPool()


def check(rc, ctx, what):
    if rc != 0:
        raise MpcxError(f"{what} failed ({rc}): {load().mpcx_last_error(ctx).decode()}")


def as_f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def dptr(a):
    return a.ctypes.data_as(_dp)


def iptr(a):
    return a.ctypes.data_as(_ip)


def lptr(a):
    return a.ctypes.data_as(_lp)


def dptr_opt(a):
    """pointer, or NULL for None"""
    return None if a is None else dptr(a)


def iptr_opt(a):
    return None if a is None else iptr(a)


def per_sat(a, S):
    """a scalar or (S,) values as the contiguous float64 (S,) array the entry points take"""
    return as_f64(np.broadcast_to(np.asarray(a, dtype=np.float64), (S,)))


def counts(a, S):
    """optional per-satellite counts (Ks, Kus, n_eval): None stays None (NULL), anything else becomes (S,) int32"""
    return None if a is None else np.ascontiguousarray(np.broadcast_to(np.asarray(a), (S,)), dtype=np.int32)


def thrust_law(law, S):
    """law = (kind, vec, Ku, end_tau) with per-satellite or broadcastable parameters -> (kind, vec, Ku, end_tau) as the
    propagating entry points take them: vec (S,3) CONSTANT, (S,) TANGENTIAL, (S,3,Ku) SEQUENCE, None otherwise; end_tau (S,)
    for SEQUENCE and None otherwise"""
    kind, vec, Ku, end_tau = law
    if kind == CTRL_CONSTANT:
        vec = as_f64(np.broadcast_to(np.asarray(vec, dtype=np.float64).reshape(-1, 3), (S, 3)))
    elif kind == CTRL_TANGENTIAL:
        vec = per_sat(np.asarray(vec, dtype=np.float64).reshape(-1), S)
    elif kind == CTRL_SEQUENCE:
        vec = np.asarray(vec, dtype=np.float64)
        vec = as_f64(np.broadcast_to(vec if vec.ndim == 3 else vec[None], (S, 3, Ku)))
    else:
        vec = None
    return kind, vec, int(Ku), per_sat(end_tau, S) if kind == CTRL_SEQUENCE else None


def model_flags(include_drag, include_J2, atmosphere=None):
    """the dynamics flags; atmosphere (not None): FLAG_ATMO beside the drag -- without drag there is nothing for it to act on"""
    return (FLAG_DRAG if include_drag else 0) | (FLAG_J2 if include_J2 else 0) | (FLAG_ATMO if include_drag and atmosphere is not None else 0)


def discretize_flags(include_drag, include_J2, uniform_steps=0, rk23=False, atmosphere=None):
    """flags of the discretize / fused-step entry points (include/mpcx.h): the model, Discretizer.use_uniform_steps with
    integrator_steps = uniform_steps (0: adaptive steps), ivp_solver = 'RK23'"""
    flags = model_flags(include_drag, include_J2, atmosphere)
    if uniform_steps:
        flags |= FLAG_UNIFORM_STEPS | (int(uniform_steps) << 8)
    if rk23:
        flags |= FLAG_RK23
    return flags


def call(name, *args, popts=None):
    """Call entry point `name` with args (the context first) and raise MpcxError unless it returns 0.  popts: a per-satellite
    option table -- the call is then the entry point's `_sat` twin, the table's pointer directly after the options pointer.
    The function is looked up on the library at call time (callers may wrap an entry point, e.g. to time it)."""
    if popts is not None:
        i = _SIGS[name][1].index(_po) + 1
        name, args = name + "_sat", (*args[:i], dptr(popts), *args[i:])
    check(getattr(load(), name)(*args), args[0], name)


SOLVER_KEYWORDS = ("tol", "acceptable_tol", "max_iter", "acceptable_iter", "n_refine", "flags")
SOLVE_INDEX_ORDER, SOLVE_LINEAR_VT, SOLVE_FIXED_TF, SOLVE_SHARED_TF, SOLVE_ONE_WAVE, SOLVE_NO_LDS, SOLVE_TIME_PARALLEL = 1, 2, 4, 8, 16, 32, 64      # mpcx_solve_opts.flags (include/mpcx.h)
SOLVE_TP_SELFTEST_DEAD = 1 << 30


def check_solver_keywords(solver):
    bad = sorted(set(solver) - set(SOLVER_KEYWORDS))
    if bad:
        raise TypeError(f"unknown solver option(s) {bad}; known: {list(SOLVER_KEYWORDS)}")


# per-satellite problem options (include/mpcx.h, MPCX_PO_*): the columns of the table, = mpcx_solve_opts' first eleven doubles
PO_MIN_MASS, PO_U_MAX, PO_R_MIN, PO_R_MAX, PO_EPS_R, PO_EPS_VR, PO_EPS_VN, PO_EPS_VT, PO_TF_MAX, PO_W_NU, PO_W_TR, NPOPT = range(12)
PO_FIELDS = ("min_mass", "u_max", "r_min", "r_max", "eps_r", "eps_vr", "eps_vn", "eps_vt", "tf_max", "w_nu", "w_tr")
_PO_SCALAR_KEYS = ("min_mass", "eps_r", "eps_vr", "eps_vn", "eps_vt", "tf_max", "w_nu", "w_tr")
_PO_DEFAULTS = (0.1, 5.0, 0.99, 5.0, 0.01, 1e-5, 1e-5, 1e-5, 5.0, 1000.0, 0.002)        # mpcx_default_solve_opts (optimizer.py:178-188)


def per_satellite_keys(options):
    """the problem options of `options` that are given per satellite: (S,) arrays, or (S, 2) for u_lim / r_lim"""
    out = []
    for k, v in (options or {}).items():
        if k in _PO_SCALAR_KEYS and np.ndim(v) >= 1:
            out.append(k)
        elif k in ("u_lim", "r_lim") and np.ndim(v) >= 2:
            out.append(k)
    return out


def make_popts(options, S):
    """The per-satellite option table of a call for S satellites (include/mpcx.h, popts [S][MPCX_NPOPT]): None when every
    problem option of `options` is a scalar (the call is then the one without a table, with its bits), otherwise a
    C-contiguous (S, 11) float64 array, scalars and defaults broadcast.  min_mass, eps_r, eps_vr, eps_vn, eps_vt, tf_max, w_nu,
    w_tr: a scalar or shape (S,); u_lim, r_lim: (2,) or (S, 2).  Any other shape raises ValueError."""
    options = options or {}
    if not per_satellite_keys(options):
        return None
    S = int(S)
    tab = np.empty((S, NPOPT), dtype=np.float64)
    tab[:] = _PO_DEFAULTS

    def column(key, v):
        v = np.asarray(v, dtype=np.float64)
        if v.ndim == 0:
            return v
        if v.shape != (S,):
            raise ValueError(f"options[{key!r}]: expected a scalar or shape ({S},), got {v.shape}")
        return v
    for key in _PO_SCALAR_KEYS:
        if key in options:
            tab[:, PO_FIELDS.index(key)] = column(key, options[key])
    for key, cols in (("u_lim", (None, PO_U_MAX)), ("r_lim", (PO_R_MIN, PO_R_MAX))):
        if key in options:
            v = np.asarray(options[key], dtype=np.float64)
            if v.shape not in ((2,), (S, 2)):
                raise ValueError(f"options[{key!r}]: expected shape (2,) or ({S}, 2), got {v.shape}")
            for j, c in enumerate(cols):
                if c is not None:
                    tab[:, c] = v[..., j]
    return np.ascontiguousarray(tab)


def scalar_options(options):
    """`options` with every per-satellite entry replaced by its first satellite's value: the scalar mpcx_solve_opts that goes
    with a table (which overrides all eleven problem options for every satellite)"""
    out = dict(options or {})
    for k in per_satellite_keys(out):
        out[k] = np.asarray(out[k], dtype=np.float64)[0].tolist()
    return out


def refuse_per_satellite(options, who):
    keys = per_satellite_keys(options)
    if keys:
        raise ValueError(f"{who}: per-satellite options {sorted(keys)} are not possible here (one final time for all satellites "
                         "cannot have per-satellite limits); pass scalars")


# reference option keys (optimizer.py:178-188) -> mpcx_solve_opts
def make_solve_opts(options=None, **solver):
    """options: dict with the reference's keys (min_mass, u_lim, r_lim, eps_r, eps_vr, eps_vn, tf_max, w_nu, w_tr;
    r_des is passed per satellite); solver: tol, acceptable_tol, max_iter, acceptable_iter, n_refine.  Per-satellite entries
    (make_popts) go into the table of the call; the struct then carries the first satellite's values."""
    o = SolveOpts()
    load().mpcx_default_solve_opts(C.byref(o))
    options = scalar_options(options)
    if "min_mass" in options: o.min_mass = options["min_mass"]
    if "u_lim" in options: o.u_max = options["u_lim"][1]
    if "r_lim" in options: o.r_min, o.r_max = options["r_lim"][0], options["r_lim"][1]
    for k in ("eps_r", "eps_vr", "eps_vn", "eps_vt", "tf_max", "w_nu", "w_tr"):
        if k in options: setattr(o, k, options[k])
    check_solver_keywords(solver)
    for k, v in solver.items():
        setattr(o, k, v)
    return o
