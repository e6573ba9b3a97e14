"""Device-pointer solves with every "don't care" byte in the caller's hands (tests/test_stale_memory_gpu.py).

The _dev entry points of include/mpcx.h work in a workspace the caller supplies and write into result buffers the caller
allocates.  The wrappers below keep every device buffer in a torch tensor (as test_two_solves_of_one_context_on_two_streams does
by hand), take the workspace tensor and the pre-fill of the result tensors from the caller, and return the results as numpy
arrays together with the workspace tensor as the call left it."""
import ctypes as C

import numpy as np

FIELDS = ("X", "U", "NU", "tf", "kkt", "status", "iters", "n_regularised", "first_regularised")

# solve_layout.hpp: the slot of one satellite in the solver workspace, in doubles.  The library exports only byte counts of whole
# workspaces; the copy below is held to them by check_layout().
_IT_N, _NS_N, _NB_N, _FAC_N, _CH_N, _NCH, _TR_N, _GL_N, _CHX_N, _TP_MAIL_N, _TP_MAXSEG, _TP_XCH_N = 66, 52, 35, 200, 104, 8, 17, 24, 10, 16, 4, 256
STAGE_DOUBLES = 105


def ws_doubles(K):
    KP = (K + 15) & ~15
    n = KP * (3 * _IT_N + _NS_N + STAGE_DOUBLES + 3) + K * (_NB_N + _FAC_N + _CH_N + _NCH * _TR_N) + 3 * _GL_N + 64
    return (n + 15) & ~15


def tp_mail_offset(K):
    return ws_doubles(K) + K * (_CHX_N + _NCH * _TR_N)


def ws_doubles_tp(K):
    return (tp_mail_offset(K) + _TP_MAIL_N + _TP_MAXSEG * _TP_XCH_N + 15) & ~15


def _env():
    import torch
    from mpconstellation_amd import _ffi
    return torch, _ffi, _ffi.load(), _ffi.context(0), torch.device("cuda", 0)


def check_layout(K):
    """the Python copy of the slot sizes is the library's"""
    _, _, lib, ctx, _ = _env()
    assert lib.mpcx_solve_workspace_bytes(3, K) == 3 * ws_doubles_tp(K) * 8
    assert lib.mpcx_solve_workspace_bytes_ctx(ctx, 200, K) == 200 * ws_doubles(K) * 8      # (above the time-parallel kernel's batch limit)


def n_slots():
    """persistent workgroups of a launch on this device = workspace slots a large batch shares (2048 on an MI355X)"""
    _, _, lib, ctx, _ = _env()
    return int(lib.mpcx_solve_workspace_bytes_ctx(ctx, 1 << 20, 3)) // (ws_doubles(3) * 8)


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _stream(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a, dtype=None):
    """numpy -> device tensor (float64 unless said otherwise); tensors pass through"""
    torch, _, _, _, d = _env()
    if isinstance(a, torch.Tensor):
        return a
    a = np.ascontiguousarray(a)
    if dtype is None:
        dtype = torch.int32 if a.dtype.kind in "iu" else torch.float64
    return torch.tensor(a, dtype=dtype, device=d)


def solver_workspace_doubles(S, K):
    """doubles of a solver workspace that serves every kernel the dispatcher may take for (S, K): one slot per satellite,
    at most one per persistent workgroup"""
    _, _, lib, ctx, _ = _env()
    return int(lib.mpcx_solve_workspace_bytes_ctx(ctx, S, K)) // 8 + 16


def step_header_doubles(S, K):
    """the fused step's workspace is [stage records | int32 discretize status | solver workspace] (solve_api.hip)"""
    return S * (K - 1) * STAGE_DOUBLES + (S + 1) // 2 + 1


def step_workspace_doubles(S, K):
    return step_header_doubles(S, K) + solver_workspace_doubles(S, K)


def filled(n, fill):
    """workspace tensor of n doubles: 'zero', 'big' (alternating +-1e300), 'inf', 'nan+' / 'nan-' (the all-ones quiet NaN
    of a 0xFF memset, and the same payload with the sign bit clear)"""
    torch, _, _, _, d = _env()
    if fill == "zero":
        return torch.zeros(n, dtype=torch.float64, device=d)
    if fill == "big":
        t = torch.full((n,), 1e300, dtype=torch.float64, device=d)
        t[1::2] = -1e300
        return t
    if fill == "inf":
        return torch.full((n,), float("inf"), dtype=torch.float64, device=d)
    if fill == "nan-":
        return torch.full((n,), -1, dtype=torch.int64, device=d).view(torch.float64)            # 0xFF bytes
    if fill == "nan+":
        return torch.full((n,), 0x7FFFFFFFFFFFFFFF, dtype=torch.int64, device=d).view(torch.float64)
    raise ValueError(fill)


def bits(t):
    import torch
    return t.view(torch.int64)


class Outputs:
    """result tensors of a solve, pre-filled: doubles with quiet NaN, status / iters / the regularisation record with -1"""

    def __init__(self, S, K):
        torch, _, _, _, d = _env()
        nan = lambda *sh: torch.full(sh, float("nan"), dtype=torch.float64, device=d)
        self.X, self.U, self.NU = nan(S, 7, K), nan(S, 3, K), nan(S, 7, K)
        self.tf, self.kkt = nan(S), nan(S)
        self.status = torch.full((S,), -1, dtype=torch.int32, device=d)
        self.iters = torch.full((S,), -1, dtype=torch.int32, device=d)
        self.reg = torch.full((S, 2), -1, dtype=torch.int32, device=d)

    def numpy(self):
        r = {k: getattr(self, k).cpu().numpy() for k in ("X", "U", "NU", "tf", "kkt", "status", "iters")}
        reg = self.reg.cpu().numpy()
        r["n_regularised"], r["first_regularised"] = reg[:, 0].copy(), reg[:, 1].copy()
        return r


def make_opts(options=None, flags=0, **solver):
    _, _ffi, _, _, _ = _env()
    return _ffi.make_solve_opts(options or {}, flags=flags, **solver)


def discretize_stages(x, u, tf, consts, Ks=None, Kus=None, flags=0, max_step=1e-2, stage=None):
    """mpcx_discretize_stages_ragged_dev -> (stage tensor [S][K-1][105], status numpy).  `stage`: the pre-filled output tensor."""
    torch, _ffi, lib, ctx, d = _env()
    x, u = dev(x), dev(u)
    S, _, K = x.shape
    Ku = u.shape[2]
    if stage is None:
        stage = torch.full((S, K - 1, STAGE_DOUBLES), float("nan"), dtype=torch.float64, device=d)
    st = torch.full((S,), -1, dtype=torch.int32, device=d)
    dKs = None if Ks is None else dev(Ks, torch.int32)
    dKus = None if Kus is None else dev(Kus, torch.int32)
    hold = [dev(tf), dev(consts)]
    _ffi.check(lib.mpcx_discretize_stages_ragged_dev(ctx, S, K, _p(dKs), Ku, _p(dKus), _p(x), _p(u), _p(hold[0]), _p(hold[1]), int(flags),
                                                     float(max_step), _p(stage), _p(st), _stream(torch)), ctx, "discretize_stages_ragged_dev")
    torch.cuda.synchronize()
    return stage, st.cpu().numpy()


def unpack_stage(stage, s, K):
    """the K - 1 stage records [A | Bn | Bp | Sigma | xi] of satellite s as the arrays of the reference layout"""
    rec = stage[s, :K - 1].cpu().numpy()
    return dict(A=rec[:, 0:49].reshape(K - 1, 7, 7), Bn=rec[:, 49:70].reshape(K - 1, 7, 3), Bp=rec[:, 70:91].reshape(K - 1, 7, 3),
                Sigma=np.ascontiguousarray(rec[:, 91:98].T), xi=np.ascontiguousarray(rec[:, 98:105].T))


def solve_dev(stage, x, u, tf, consts, r_des, opts, Ks=None, ws=None, out=None):
    """mpcx_solve_batch_ragged_dev in the caller's workspace tensor `ws` -> (results dict of numpy arrays, ws, out)"""
    torch, _ffi, lib, ctx, d = _env()
    x, u, stage = dev(x), dev(u), dev(stage)
    S, _, K = x.shape
    ws = filled(solver_workspace_doubles(S, K), "zero") if ws is None else ws
    assert ws.dtype == torch.float64 and ws.is_contiguous() and ws.numel() >= solver_workspace_doubles(S, K)
    out = out or Outputs(S, K)
    dKs = None if Ks is None else dev(Ks, torch.int32)
    hold = [dev(tf), dev(consts), dev(r_des)]
    st = _stream(torch)
    _ffi.check(lib.mpcx_solve_batch_ragged_dev(ctx, S, K, _p(dKs), _p(stage), _p(x), _p(u), _p(hold[0]), _p(hold[1]), _p(hold[2]), C.byref(opts),
                                               _p(out.X), _p(out.U), _p(out.NU), _p(out.tf), _p(out.status), _p(out.iters), _p(out.kkt),
                                               _p(ws), st), ctx, "solve_batch_ragged_dev")
    _ffi.check(lib.mpcx_solve_regularised_dev(ctx, S, _p(out.reg), st), ctx, "solve_regularised_dev")
    torch.cuda.synchronize()
    return out.numpy(), ws, out


def step_dev(x, u, tf, consts, r_des, opts, Ks=None, flags=0, max_step=1e-2, ws=None, out=None):
    """mpcx_mpc_step_batch_ragged_dev in the caller's workspace tensor `ws` -> (results dict of numpy arrays, ws, out)"""
    torch, _ffi, lib, ctx, d = _env()
    x, u = dev(x), dev(u)
    S, _, K = x.shape
    ws = filled(step_workspace_doubles(S, K), "zero") if ws is None else ws
    assert ws.dtype == torch.float64 and ws.is_contiguous() and ws.numel() >= step_workspace_doubles(S, K)
    out = out or Outputs(S, K)
    dKs = None if Ks is None else dev(Ks, torch.int32)
    hold = [dev(tf), dev(consts), dev(r_des)]
    st = _stream(torch)
    _ffi.check(lib.mpcx_mpc_step_batch_ragged_dev(ctx, S, K, _p(dKs), _p(x), _p(u), _p(hold[0]), _p(hold[1]), _p(hold[2]), int(flags),
                                                  float(max_step), C.byref(opts), _p(out.X), _p(out.U), _p(out.NU), _p(out.tf), _p(out.status),
                                                  _p(out.iters), _p(out.kkt), _p(ws), st), ctx, "mpc_step_batch_ragged_dev")
    _ffi.check(lib.mpcx_solve_regularised_dev(ctx, S, _p(out.reg), st), ctx, "solve_regularised_dev")
    torch.cuda.synchronize()
    return out.numpy(), ws, out


def propagate_thrust_dev(y0, tf, consts, table, end_tau, n_eval, n_evals=None, Kus=None, flags=0, max_step=1e-3):
    """mpcx_propagate_thrust_batch_ragged_dev with a SEQUENCE table [S][3][Ku]; y_out / u_out pre-filled with NaN"""
    torch, _ffi, lib, ctx, d = _env()
    table = dev(table)
    S, _, Ku = table.shape
    y = torch.full((S, 7, n_eval), float("nan"), dtype=torch.float64, device=d)
    uo = torch.full((S, 3, n_eval), float("nan"), dtype=torch.float64, device=d)
    st = torch.full((S,), -1, dtype=torch.int32, device=d); ns = torch.full((S,), -1, dtype=torch.int32, device=d)
    dn = None if n_evals is None else dev(n_evals, torch.int32)
    dk = None if Kus is None else dev(Kus, torch.int32)
    hold = [dev(y0), dev(tf), dev(consts), dev(end_tau)]
    _ffi.check(lib.mpcx_propagate_thrust_batch_ragged_dev(ctx, S, int(n_eval), _p(dn), _p(hold[0]), _p(hold[1]), _p(hold[2]), int(flags),
                                                          _ffi.CTRL_SEQUENCE, _p(table), Ku, _p(dk), _p(hold[3]), float(max_step), _p(y), _p(uo),
                                                          _p(st), _p(ns), _stream(torch)), ctx, "propagate_thrust_batch_ragged_dev")
    torch.cuda.synchronize()
    return y.cpu().numpy(), uo.cpu().numpy(), st.cpu().numpy(), ns.cpu().numpy()


def same_bits(a, b):
    """bit-for-bit equality of two numpy arrays (NaNs compare by payload)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return a.tobytes() == b.tobytes()
