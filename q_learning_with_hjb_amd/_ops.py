"""Typed, tensor-level wrappers over the C ABI: torch CUDA tensors in, torch CUDA tensors out.

PyTorch is plumbing here (device memory + the current HIP stream); every computation below is one
of the hand-written gfx950 kernels in csrc/.  Inputs must be float32/float64 CUDA tensors; the
public `Dynamics` / `Controller` classes do the numpy <-> device marshalling around these.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import threading

import torch

from . import _abi
from ._abi import check, lib, ref


def require_device() -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("hjbx: no HIP device visible -- the batched rollout / HJB path only runs on an MI355X "
                           "(there is deliberately no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _sfx(t: torch.Tensor) -> str:
    if t.dtype == torch.float32:
        return "f32"
    if t.dtype == torch.float64:
        return "f64"
    raise TypeError(f"hjbx kernels take float32 or float64 tensors, got {t.dtype}")


def _chk(t: torch.Tensor, name: str, shape, dtype=None):
    if not t.is_cuda:
        raise TypeError(f"{name} must be a CUDA (HIP) tensor")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name} has dtype {t.dtype}, expected {dtype}")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


class Workspaces:
    """The library's device scratch for one device, each buffer allocated on first use: the arrival tickets of the reducing entry points
    (`reduce`), the work-distribution words of the persistent rollout kernel (`rollout`), the parameter-gradient scratch (`grad`) and the
    slice offsets of the replay append (`append`).
    Tickets and words are zero-filled ONCE; every launch that runs to completion leaves them at zero (include/hjbx.h).

    `owned=True` is the set of a captured graph, which replays into the raw pointers of whatever the capture was handed: it never frees
    or replaces a buffer it has handed out.  The eager sets of `_workspaces` (`owned=False`) give a much larger gradient scratch back."""

    def __init__(self, device, owned=True):
        self.device, self.owned = torch.device(device), owned
        self._reduce = self._rollout = self._grad = self._append = None
        self._retired = []

    def reduce(self) -> torch.Tensor:
        if self._reduce is None:
            self._reduce = torch.zeros((lib().hjbx_reduce_workspace_bytes() + 15) // 16 * 2, dtype=torch.float64, device=self.device)
        return self._reduce

    def rollout(self) -> torch.Tensor:
        if self._rollout is None:
            self._rollout = torch.zeros((lib().hjbx_rollout_workspace_bytes() + 15) // 16 * 4, dtype=torch.int32, device=self.device)
        return self._rollout

    def grad(self, need: int) -> torch.Tensor:
        """At least `need` bytes of uninitialised scratch: grown on demand; an eager set also gives a much larger one back."""
        ws = self._grad
        if ws is None or ws.numel() < need or (not self.owned and ws.numel() > 4 * need + (64 << 20)):
            if self.owned and ws is not None:
                self._retired.append(ws)          # a graph captured with it may still replay into it
            ws = self._grad = None                # (an eager set hands the old buffer back to the allocator before taking the new one)
            ws = self._grad = torch.empty((need + 255) // 256 * 256, dtype=torch.uint8, device=self.device)
        return ws

    def append(self, need: int) -> torch.Tensor:
        """At least `need` bytes of uninitialised scratch for hjbx_replay_append_*: grown on demand (4 bytes per 21 environments: never worth
        giving back)."""
        ws = self._append
        if ws is None or ws.numel() < need:
            if self.owned and ws is not None:
                self._retired.append(ws)
            ws = self._append = torch.empty((need + 255) // 256 * 256, dtype=torch.uint8, device=self.device)
        return ws


_eager = {}                  # (device index, stream handle) -> the Workspaces of eager launches on that stream
_active = threading.local()


@contextlib.contextmanager
def using_workspaces(ws: Workspaces):
    """Inside the block, every call on this thread takes its workspaces from `ws` (a capture owner's set) instead of the eager set of its
    stream.  Thread-local is enough: the workspaces are only requested by forward code on the calling thread -- the backward passes of
    _HJBResidualSum and _TerminationResidualSum, which autograd may run on another thread, only multiply saved tensors."""
    prev = getattr(_active, "ws", None)
    _active.ws = ws
    try:
        yield ws
    finally:
        _active.ws = prev


def _workspaces(device) -> Workspaces:
    """The set an `_ops` call on `device` passes to its kernel: the one `using_workspaces` activated, else the eager set of the stream
    the call launches on."""
    ws = getattr(_active, "ws", None)
    if ws is not None:
        return ws
    key = (device.index, _stream())
    ws = _eager.get(key)
    if ws is None:
        ws = _eager[key] = Workspaces(device, owned=False)
    return ws


def _rollout_workspace(device) -> torch.Tensor:
    """The work-distribution words the persistent rollout kernel launched now on `device` gets (tests read them to check they are left zeroed)."""
    return _workspaces(device).rollout()


def _fn(name, t):
    return getattr(lib(), f"hjbx_{name}_{_sfx(t)}")


def affine(sys, x):
    B = x.shape[0]
    _chk(x, "x", (B, sys.n))
    f1 = torch.empty_like(x)
    f2 = torch.empty((B, sys.n, sys.m), dtype=x.dtype, device=x.device)
    check(_fn("affine", x)(sys.ptr, _p(x), _p(f1), _p(f2), B, _stream()))
    return f1, f2


def wrap(sys, x, out=None):
    B = x.shape[0]
    _chk(x, "x", (B, sys.n))
    out = torch.empty_like(x) if out is None else out
    _chk(out, "out", (B, sys.n), x.dtype)
    check(_fn("wrap", x)(sys.ptr, _p(x), _p(out), B, _stream()))
    return out


def dynamics_step(sys, x, u):
    B = x.shape[0]
    _chk(x, "x", (B, sys.n))
    _chk(u, "u", (B, sys.m), x.dtype)
    xd = torch.empty_like(x)
    check(_fn("dynamics_step", x)(sys.ptr, _p(x), _p(u), _p(xd), B, _stream()))
    return xd


def simulate(sys, x, u, integrator=_abi.EULER, out=None):
    B = x.shape[0]
    _chk(x, "x", (B, sys.n))
    _chk(u, "u", (B, sys.m), x.dtype)
    out = torch.empty_like(x) if out is None else out
    _chk(out, "out", (B, sys.n), x.dtype)
    check(_fn("simulate", x)(sys.ptr, int(integrator), _p(x), _p(u), _p(out), B, _stream()))
    return out


def initial_state(sys, x0_mean, x0_std, u01):
    import numpy as np
    B = u01.shape[0]
    _chk(u01, "u01", (B, sys.n))
    mean = np.ascontiguousarray(x0_mean, np.float64).reshape(sys.n)
    std = np.ascontiguousarray(x0_std, np.float64).reshape(sys.n)
    x0 = torch.empty_like(u01)
    check(_fn("initial_state", u01)(sys.ptr, mean.ctypes.data, std.ctypes.data, _p(u01), _p(x0), B, _stream()))
    return x0


def initial_state_philox(sys, x0_mean, x0_std, batch_size, seed, first_row=0, dtype=torch.float32, out=None, device=None):
    """hjbx_initial_state_philox_*: (B, n) start states whose uniforms the kernel draws itself -- row i from (seed, first_row + i) alone
    (Philox4x32-10; the stream is defined in include/hjbx.h).  seed and first_row are unsigned 64-bit."""
    import numpy as np
    B, seed, first_row = int(batch_size), int(seed), int(first_row)
    if B < 0:
        raise ValueError(f"batch_size must be non-negative, got {B}")
    if not 0 <= seed < 1 << 64 or not 0 <= first_row < 1 << 64:
        raise ValueError("seed and first_row must fit an unsigned 64-bit integer")
    if first_row + B > 1 << 64:
        raise ValueError("first_row + batch_size runs past the end of the stream (2^64 rows)")
    mean = np.ascontiguousarray(x0_mean, np.float64).reshape(sys.n)
    std = np.ascontiguousarray(x0_std, np.float64).reshape(sys.n)
    if out is None:
        out = torch.empty((B, sys.n), dtype=dtype, device=require_device() if device is None else device)
    _chk(out, "out", (B, sys.n), dtype)
    check(_fn("initial_state_philox", out)(sys.ptr, mean.ctypes.data, std.ctypes.data, seed, first_row, _p(out), B, _stream()))
    return out


def rollout_cost_stats(cost, done_step, want_traj_cost=True):
    """hjbx_rollout_cost_stats_*: cost (S, B) time-major log, done_step (B,) int32 -> (traj_cost (B,) float64 or None, stats (4,) float64
    on the device = {sum c, sum (c - mean)^2, sum (done_step + 1), B}); tuples past done_step are never read."""
    if cost.dim() != 2:
        raise ValueError(f"cost must be the (S, B) log, got shape {tuple(cost.shape)}")
    S, B = cost.shape
    _sfx(cost)
    _chk(cost, "cost", (S, B))
    _chk(done_step, "done_step", (B,), torch.int32)
    if S < 1:
        raise ValueError("cost must hold at least one time step")
    traj_cost = torch.empty((B,), dtype=torch.float64, device=cost.device) if want_traj_cost else None
    stats = torch.zeros((4,), dtype=torch.float64, device=cost.device)
    ws = _workspaces(cost.device).reduce()
    check(_fn("rollout_cost_stats", cost)(_p(cost), _p(done_step), S, B, _p(traj_cost), _p(stats), _p(ws), _stream()))
    return traj_cost, stats


def activation_probe(activation, a, want_h=True, want_s=True):
    """hjbx_activation_probe_f32 (TEST INFRASTRUCTURE): the matrix-core kernels' own activation code on a flat float32 tensor `a` ->
    (h = act(a), s = the derivative factor as the kernels form it: [h > 0], 1 - h^2, or the cosine next to the sine)."""
    N = a.numel()
    _chk(a, "a", (N,), torch.float32)
    h = torch.empty_like(a) if want_h else None
    s = torch.empty_like(a) if want_s else None
    check(lib().hjbx_activation_probe_f32(_abi._ACTIVATIONS[activation], _p(a), _p(h), _p(s), N, _stream()))
    return h, s


def running_cost(sys, task, x, u):
    B = x.shape[0]
    _chk(x, "x", (B, sys.n))
    _chk(u, "u", (B, sys.m), x.dtype)
    c = torch.empty((B,), dtype=x.dtype, device=x.device)
    check(_fn("running_cost", x)(sys.ptr, ref(task), _p(x), _p(u), _p(c), B, _stream()))
    return c


def termination_cost(sys, task, x):
    B = x.shape[0]
    _chk(x, "x", (B, sys.n))
    c = torch.empty((B,), dtype=x.dtype, device=x.device)
    check(_fn("termination_cost", x)(sys.ptr, ref(task), _p(x), _p(c), B, _stream()))
    return c


def control_from_grad(sys, task, x, grad_v):
    B = x.shape[0]
    _chk(x, "x", (B, sys.n))
    _chk(grad_v, "grad_v", (B, sys.n), x.dtype)
    u = torch.empty((B, sys.m), dtype=x.dtype, device=x.device)
    check(_fn("control_from_grad", x)(sys.ptr, ref(task), _p(x), _p(grad_v), _p(u), B, _stream()))
    return u


def hjb_residual(sys, task, x, grad_v, done, mode=_abi.RESIDUAL_NORMALISED, want_loss=True, want_grad=True, want_sums=True):
    """-> (loss_i (B,) | None, dloss_dgrad (B,n) | None, sums (3,) | None)"""
    B = x.shape[0]
    _chk(x, "x", (B, sys.n))
    _chk(grad_v, "grad_v", (B, sys.n), x.dtype)
    _chk(done, "done", (B,), x.dtype)
    li = torch.empty((B,), dtype=x.dtype, device=x.device) if want_loss else None
    dg = torch.empty_like(x) if want_grad else None
    sums = torch.empty((3,), dtype=x.dtype, device=x.device) if want_sums else None
    ws = _workspaces(x.device).reduce() if want_sums else None
    check(_fn("hjb_residual", x)(sys.ptr, ref(task), int(mode), _p(x), _p(grad_v), _p(done), _p(li), _p(dg), _p(sums),
                                 _p(ws), B, _stream()))
    return li, dg, sums


def termination_residual(eps, V, cost, done, want_loss=True, want_grad=True, want_sums=True):
    B = V.shape[0]
    _chk(V, "V", (B,))
    _chk(cost, "cost", (B,), V.dtype)
    _chk(done, "done", (B,), V.dtype)
    li = torch.empty_like(V) if want_loss else None
    dv = torch.empty_like(V) if want_grad else None
    sums = torch.empty((3,), dtype=V.dtype, device=V.device) if want_sums else None
    ws = _workspaces(V.device).reduce() if want_sums else None
    check(_fn("termination_residual", V)(float(eps), _p(V), _p(cost), _p(done), _p(li), _p(dv), _p(sums), _p(ws), B, _stream()))
    return li, dv, sums


def vhjb_step(sys, task, t, T_max, x, grad_v, x_next, cost_t, done_t, done_step, u_out=None, integrator=_abi.EULER, resid_t=None):
    B = x.shape[0]
    _chk(x, "x", (B, sys.n))
    _chk(grad_v, "grad_v", (B, sys.n), x.dtype)
    _chk(x_next, "x_next", (B, sys.n), x.dtype)
    _chk(cost_t, "cost_t", (B,), x.dtype)
    _chk(done_t, "done_t", (B,), x.dtype)
    _chk(done_step, "done_step", (B,), torch.int32)
    if u_out is not None:
        _chk(u_out, "u_out", (B, sys.m), x.dtype)
    if resid_t is not None:
        _chk(resid_t, "resid_t", (B,), x.dtype)
    check(_fn("vhjb_step", x)(sys.ptr, ref(task), int(integrator), int(t), int(T_max), _p(x), _p(grad_v), _p(x_next), _p(u_out),
                              _p(cost_t), _p(done_t), _p(done_step), _p(resid_t), B, _stream()))


def controller(sys, ctrl, x):
    B = x.shape[0]
    _chk(x, "x", (B, sys.n))
    u = torch.empty((B, sys.m), dtype=x.dtype, device=x.device)
    check(_fn("controller", x)(sys.ptr, ref(ctrl), _p(x), _p(u), B, _stream()))
    return u


def rollout_feedback(sys, ctrl, x0, T_steps, task=None, integrator=_abi.EULER, terminate=False, log_traj=True, log_u=False,
                     log_cost=False, stop_at_target=False):
    """Whole closed loop in one kernel launch.  Returns a dict of device tensors (time-major)."""
    B = x0.shape[0]
    _chk(x0, "x0", (B, sys.n))
    dt, dev = x0.dtype, x0.device
    traj = torch.empty((T_steps + 1, B, sys.n), dtype=dt, device=dev) if log_traj else None
    ulog = torch.empty((T_steps, B, sys.m), dtype=dt, device=dev) if log_u else None
    cost = torch.empty((T_steps + 1, B), dtype=dt, device=dev) if (log_cost and task is not None) else None
    total = torch.empty((B,), dtype=dt, device=dev) if task is not None else None
    done_step = torch.empty((B,), dtype=torch.int32, device=dev)
    x_final = torch.empty_like(x0)
    flags = (_abi.ROLLOUT_TERMINATE if terminate else 0) | (_abi.ROLLOUT_STOP_AT_TARGET if stop_at_target else 0)
    check(_fn("rollout_feedback", x0)(sys.ptr, ref(task), ref(ctrl), int(integrator), flags, int(T_steps), _p(x0), _p(traj),
                                      _p(ulog), _p(cost), _p(done_step), _p(total), _p(x_final), B, _stream()))
    return dict(traj=traj, u=ulog, cost=cost, done_step=done_step, total_cost=total, x_final=x_final)


def _env_params(ctl, w, x):
    """the (B, n_w) buffer of a user-defined law's per-environment values, or None for a law that reads none"""
    if ctl.n_env_params == 0:
        if w is not None:
            raise ValueError("this control law reads no per-environment values (device_source(): env_params=0)")
        return None
    if w is None:
        raise ValueError(f"this control law reads {ctl.n_env_params} per-environment values: pass env_params of shape (B, {ctl.n_env_params})")
    _chk(w, "env_params", (x.shape[0], ctl.n_env_params), x.dtype)
    return w


def user_controller_eval(ctl, x, t=0.0, w=None):
    """hjbx_user_controller_eval_*: u (B, m) = clip(law(x, w, t)) for a _abi.UserControllerHandle."""
    B = x.shape[0]
    _chk(x, "x", (B, ctl.n))
    w = _env_params(ctl, w, x)
    u = torch.empty((B, ctl.m), dtype=x.dtype, device=x.device)
    check(_fn("user_controller_eval", x)(ctl.ptr, _p(x), _p(w), float(t), _p(u), B, _stream()))
    return u


def user_controller_rollout(ctl, x0, T_steps, task=None, integrator=_abi.EULER, terminate=False, log_traj=True, log_u=False,
                            log_cost=False, stop_at_target=False, t0=0.0, w=None):
    """rollout_feedback under a user-defined control law (hjbx_user_controller_rollout_*): one kernel launch, the same dict of time-major
    device tensors.  The law sees the time t0 + k dt at step k and row b of `w` (B, n_w) in environment b."""
    B = x0.shape[0]
    _chk(x0, "x0", (B, ctl.n))
    w = _env_params(ctl, w, x0)
    dt, dev = x0.dtype, x0.device
    traj = torch.empty((T_steps + 1, B, ctl.n), dtype=dt, device=dev) if log_traj else None
    ulog = torch.empty((T_steps, B, ctl.m), dtype=dt, device=dev) if log_u else None
    cost = torch.empty((T_steps + 1, B), dtype=dt, device=dev) if (log_cost and task is not None) else None
    total = torch.empty((B,), dtype=dt, device=dev) if task is not None else None
    done_step = torch.empty((B,), dtype=torch.int32, device=dev)
    x_final = torch.empty_like(x0)
    flags = (_abi.ROLLOUT_TERMINATE if terminate else 0) | (_abi.ROLLOUT_STOP_AT_TARGET if stop_at_target else 0)
    check(_fn("user_controller_rollout", x0)(ctl.ptr, ref(task), int(integrator), flags, float(t0), int(T_steps), _p(x0), _p(w), _p(traj),
                                             _p(ulog), _p(cost), _p(done_step), _p(total), _p(x_final), B, _stream()))
    return dict(traj=traj, u=ulog, cost=cost, done_step=done_step, total_cost=total, x_final=x_final)


def _chk_plan(coeff, cum_t, end_pt, B):
    """-> (S, n_plans) of a device plan: coeff (n_plans, 2, S, 8), cum_t (n_plans, S + 1) float64, end_pt (n_plans, 2); n_plans in {1, B}"""
    _sfx(coeff)
    if coeff.dim() != 4 or coeff.shape[1] != 2 or coeff.shape[3] != 8 or coeff.shape[2] < 1:
        raise ValueError(f"coeff must be (n_plans, 2, S >= 1, 8), got shape {tuple(coeff.shape)}")
    n_plans, S = coeff.shape[0], coeff.shape[2]
    if n_plans != 1 and n_plans != B:
        raise ValueError(f"{n_plans} plans for {B} environments: a plan is shared (1) or there is one per environment")
    _chk(coeff, "coeff", (n_plans, 2, S, 8))
    _chk(cum_t, "cum_t", (n_plans, S + 1), torch.float64)
    _chk(end_pt, "end_pt", (n_plans, 2), coeff.dtype)
    return S, n_plans


def minsnap_reference(sys, coeff, cum_t, end_pt, T_steps, t0=0.0, B=None):
    """hjbx_minsnap_reference_*: the planner's update(t0 + k dt) for k < T_steps on the plan(s) `coeff` / `cum_t` / `end_pt` (see _chk_plan;
    B defaults to the number of plans) -> time-major x_ref (T_steps, B, 6), u_ref (T_steps, B, 2) of coeff's dtype."""
    B = coeff.shape[0] if B is None else int(B)
    S, n_plans = _chk_plan(coeff, cum_t, end_pt, B)
    T_steps = int(T_steps)
    x_ref = torch.empty((max(T_steps, 0), B, 6), dtype=coeff.dtype, device=coeff.device)
    u_ref = torch.empty((max(T_steps, 0), B, 2), dtype=coeff.dtype, device=coeff.device)
    check(_fn("minsnap_reference", coeff)(sys.ptr, _p(coeff), _p(cum_t), _p(end_pt), S, n_plans, float(t0), T_steps, _p(x_ref), _p(u_ref), B, _stream()))
    return x_ref, u_ref


def rollout_minsnap_tracking(sys, ctrl, coeff, cum_t, end_pt, x0, T_steps, t0=0.0, task=None, integrator=_abi.EULER, log_traj=True, log_u=True,
                             log_cost=False, log_reference=False):
    """hjbx_rollout_minsnap_tracking_*: the closed loop u = clip(u_ref(t) - K wrap(x - x_ref(t))) along a min-snap plan in one kernel launch.
    Returns a dict of time-major device tensors: traj (T+1, B, 6), u (T, B, 2), cost (T, B), total_cost (B,) (both need `task`), x_final,
    x_ref (T, B, 6), u_ref (T, B, 2); None for what was not asked for."""
    B = x0.shape[0]
    _chk(x0, "x0", (B, 6))
    S, n_plans = _chk_plan(coeff, cum_t, end_pt, B)
    if coeff.dtype != x0.dtype or coeff.device != x0.device:
        raise ValueError(f"the plan is {coeff.dtype} on {coeff.device}, x0 {x0.dtype} on {x0.device}")
    T_steps = int(T_steps)
    Tn, dt, dev = max(T_steps, 0), x0.dtype, x0.device
    traj = torch.empty((Tn + 1, B, 6), dtype=dt, device=dev) if log_traj else None
    ulog = torch.empty((Tn, B, 2), dtype=dt, device=dev) if log_u else None
    cost = torch.empty((Tn, B), dtype=dt, device=dev) if (log_cost and task is not None) else None
    total = torch.empty((B,), dtype=dt, device=dev) if task is not None else None
    x_final = torch.empty_like(x0)
    xr = torch.empty((Tn, B, 6), dtype=dt, device=dev) if log_reference else None
    ur = torch.empty((Tn, B, 2), dtype=dt, device=dev) if log_reference else None
    check(_fn("rollout_minsnap_tracking", x0)(sys.ptr, ref(task), ref(ctrl), int(integrator), _p(coeff), _p(cum_t), _p(end_pt), S, n_plans, float(t0),
                                              T_steps, _p(x0), _p(traj), _p(ulog), _p(cost), _p(total), _p(x_final), _p(xr), _p(ur), B, _stream()))
    return dict(traj=traj, u=ulog, cost=cost, total_cost=total, x_final=x_final, x_ref=xr, u_ref=ur)


def value_grad(sys, mlp_desc, x, want_v=True, want_grad=True):
    """Fused MFMA value network forward + input gradient (f32 only)."""
    B = x.shape[0]
    _chk(x, "x", (B, sys.n), torch.float32)
    V = torch.empty((B,), dtype=x.dtype, device=x.device) if want_v else None
    g = torch.empty_like(x) if want_grad else None
    check(lib().hjbx_value_grad_f32(sys.ptr, ref(mlp_desc), _p(x), _p(V), _p(g), B, _stream()))
    return V, g


def value_hessian(sys, mlp_desc, x, want_hessian=True, want_jacobian=False):
    """hjbx_value_hessian_f32: H (B, n, n) = d2V/dx2 and dy_dx (B, n, h3) = d(last layer)/d(error coordinates) of the PD value network on the
    matrix cores (f32 only; None for an output that is not asked for).  The built-in systems, and a user-defined system whose handle asked
    for the matrix-core kernels (the first call for an activation compiles its kernel); NotImplementedError for a user-defined system that
    has not asked, or whose kernel the library refuses because it would need scratch."""
    B = x.shape[0]
    _chk(x, "x", (B, sys.n), torch.float32)
    H = torch.empty((B, sys.n, sys.n), dtype=x.dtype, device=x.device) if want_hessian else None
    J = torch.empty((B, sys.n, int(mlp_desc.h3)), dtype=x.dtype, device=x.device) if want_jacobian else None
    check(lib().hjbx_value_hessian_f32(sys.ptr, ref(mlp_desc), _p(x), _p(H), _p(J), B, _stream()))
    return H, J


def softpd_value_grad(sys, mlp_desc, x, want_v=True, want_grad=True):
    """value_grad for the soft-PD network (mlp_desc: _abi.HjbxSoftpdMlp): hjbx_softpd_value_grad_f32."""
    B = x.shape[0]
    _chk(x, "x", (B, sys.n), torch.float32)
    V = torch.empty((B,), dtype=x.dtype, device=x.device) if want_v else None
    g = torch.empty_like(x) if want_grad else None
    check(lib().hjbx_softpd_value_grad_f32(sys.ptr, ref(mlp_desc), _p(x), _p(V), _p(g), B, _stream()))
    return V, g


def softpd_value_hessian(sys, mlp_desc, x):
    """hjbx_softpd_value_hessian_f32: H (B, n, n) = d2V/dx2 of the soft-PD value network (mlp_desc: _abi.HjbxSoftpdMlp) on the matrix cores
    (f32 only; relu: zeros).  A user-defined system whose handle asked for the matrix-core kernels runs its own kernel, compiled at the
    first call for an activation.  ValueError for a wrong shape or dtype, NotImplementedError for what the library refuses (a user-defined
    system that has not asked or whose kernel would need scratch, a linear system with n outside {2, 4, 6})."""
    B = x.shape[0]
    if x.dtype != torch.float32:
        raise ValueError(f"x has dtype {x.dtype}, expected {torch.float32}")
    _chk(x, "x", (B, sys.n), torch.float32)
    H = torch.empty((B, sys.n, sys.n), dtype=x.dtype, device=x.device)
    check(lib().hjbx_softpd_value_hessian_f32(sys.ptr, ref(mlp_desc), _p(x), _p(H), B, _stream()))
    return H


def vhjb_rollout(sys, task, mlp_desc, x, n_steps, T_max, done_step, t_first=0, integrator=_abi.EULER, log_traj=True, log_u=False,
                 log_residual=False, want_x_out=False, env_order=None, out=None):
    """`n_steps` closed-loop VHJB steps (value gradient + step) in ONE kernel launch (f32).  `done_step` (B,) int32 is
    updated in place.  Returns a dict of time-major device tensors: traj (n_steps+1,B,n) | None, cost, done
    (n_steps,B), u (n_steps,B,m) | None, residual (n_steps,B) | None, x_out (B,n) | None.
    `env_order` (B,) int32: permutation packing the environments into the kernel's tiles (live ones first = compaction).
    `out`: dict of preallocated contiguous slabs to write into (keys traj / u / cost / done / residual, e.g. time slices of a
    whole-horizon log) instead of fresh tensors."""
    return _mfma_rollout(lib().hjbx_vhjb_rollout_f32, sys, task, mlp_desc, x, n_steps, T_max, done_step, t_first, integrator, log_traj, log_u,
                         log_residual, want_x_out, env_order, out)


def softpd_rollout(sys, task, mlp_desc, x, n_steps, T_max, done_step, t_first=0, integrator=_abi.EULER, log_traj=True, log_u=False,
                   log_residual=False, want_x_out=False, env_order=None, out=None):
    """vhjb_rollout for the soft-PD network (mlp_desc: _abi.HjbxSoftpdMlp): hjbx_softpd_rollout_f32, same arguments and results."""
    return _mfma_rollout(lib().hjbx_softpd_rollout_f32, sys, task, mlp_desc, x, n_steps, T_max, done_step, t_first, integrator, log_traj, log_u,
                         log_residual, want_x_out, env_order, out)


def _mfma_rollout(entry, sys, task, mlp_desc, x, n_steps, T_max, done_step, t_first, integrator, log_traj, log_u, log_residual, want_x_out,
                  env_order, out):
    B = x.shape[0]
    _chk(x, "x", (B, sys.n), torch.float32)
    _chk(done_step, "done_step", (B,), torch.int32)
    dev = x.device
    out = out or {}

    def slab(key, shape, wanted):
        t = out.get(key)
        if t is not None:
            _chk(t, key, shape, torch.float32)
            return t
        return torch.empty(shape, dtype=torch.float32, device=dev) if wanted else None

    traj = slab("traj", (n_steps + 1, B, sys.n), log_traj)
    ulog = slab("u", (n_steps, B, sys.m), log_u)
    cost = slab("cost", (n_steps, B), True)
    done = slab("done", (n_steps, B), True)
    resid = slab("residual", (n_steps, B), log_residual)
    x_out = torch.empty_like(x) if want_x_out else None
    if env_order is not None:
        _chk(env_order, "env_order", (B,), torch.int32)
    check(entry(sys.ptr, ref(task), ref(mlp_desc), int(integrator), int(t_first), int(n_steps), int(T_max), _p(x), _p(traj), _p(ulog), _p(cost),
                _p(done), _p(resid), _p(done_step), _p(x_out), _p(env_order), B, _p(_rollout_workspace(dev)), _stream()))
    return dict(traj=traj, u=ulog, cost=cost, done=done, residual=resid, x_out=x_out)


def value_loss_grad(sys, task, mlp_desc, x, cost, done, mode=_abi.RESIDUAL_NORMALISED, out=None):
    """Fused parameter gradient of the value-learning step (f32, relu): -> flat (2P + 4,) =
    [d sum(hjb)/dW1 | dW2 | dW3 | d sum(termination)/dW1 | dW2 | dW3 | sum hjb, sum termination, #interior, #done]."""
    B = x.shape[0]
    _chk(x, "x", (B, sys.n), torch.float32)
    _chk(cost, "cost", (B,), torch.float32)
    _chk(done, "done", (B,), torch.float32)
    P = sys.n * mlp_desc.h1 + mlp_desc.h1 * mlp_desc.h2 + mlp_desc.h2 * mlp_desc.h3
    flat = torch.empty((2 * P + 4,), dtype=torch.float32, device=x.device) if out is None else out
    _chk(flat, "out", (2 * P + 4,), torch.float32)
    ws = _workspaces(x.device).grad(lib().hjbx_value_loss_grad_workspace_bytes(B))
    check(lib().hjbx_value_loss_grad_f32(sys.ptr, ref(task), ref(mlp_desc), int(mode), _p(x), _p(cost), _p(done), _p(flat), _p(ws), B, _stream()))
    return flat


def _adam_struct(params, exp_avgs, exp_avg_sqs, steps, ticket, lr, beta1, beta2, adam_eps):
    st = _abi.HjbxAdamState()
    for i, (p, m, v, k) in enumerate(zip(params, exp_avgs, exp_avg_sqs, steps)):
        for t, nm in ((p, "param"), (m, "exp_avg"), (v, "exp_avg_sq")):
            _chk(t, nm, tuple(p.shape), torch.float32)
        _chk(k, "step", (), torch.float32)
        st.param[i], st.exp_avg[i], st.exp_avg_sq[i], st.numel[i], st.step[i] = p.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), k.data_ptr()
    _chk(ticket, "ticket", (1,), torch.int32)
    st.ticket = ticket.data_ptr()
    st.lr, st.beta1, st.beta2, st.eps = float(lr), float(beta1), float(beta2), float(adam_eps)
    return st


def _reg_args(regularization):
    if torch.is_tensor(regularization):
        _chk(regularization, "regularization", (), torch.float32)
        return _p(regularization), 0.0
    return None, float(regularization)


def next_minibatch(buf_x, buf_cost, buf_done, perm, reg_table, xs, costs, dones, reg_out):
    """struct hjbx_next_minibatch for value_loss_adam: what replay_gather would be called with for the update after this one."""
    batch, n = xs.shape
    _chk(buf_x, "buf_x", (buf_x.shape[0], n), torch.float32)
    _chk(buf_cost, "buf_cost", (buf_x.shape[0],), torch.float32)
    _chk(buf_done, "buf_done", (buf_x.shape[0],), torch.float32)
    _chk(perm, "perm", (perm.shape[0],), torch.int32)
    _chk(costs, "costs", (batch,), torch.float32)
    _chk(dones, "dones", (batch,), torch.float32)
    _chk(reg_out, "reg_out", (), torch.float32)
    _chk(reg_table, "reg_table", (reg_table.shape[0],), torch.float32)
    nx = _abi.HjbxNextMinibatch()
    nx.buf_x, nx.buf_cost, nx.buf_done, nx.capacity, nx.n = buf_x.data_ptr(), buf_cost.data_ptr(), buf_done.data_ptr(), buf_x.shape[0], n
    nx.perm, nx.perm_len, nx.reg_table, nx.table_len, nx.batch = perm.data_ptr(), perm.shape[0], reg_table.data_ptr(), reg_table.shape[0], batch
    nx.xs, nx.costs, nx.dones, nx.reg_out = xs.data_ptr(), costs.data_ptr(), dones.data_ptr(), reg_out.data_ptr()
    nx._keep = (buf_x, buf_cost, buf_done, perm, reg_table, xs, costs, dones, reg_out)       # the struct holds raw pointers
    return nx


def value_loss_adam(sys, task, mlp_desc, x, cost, done, mode, regularization, eps, params, exp_avgs, exp_avg_sqs, steps, ticket, lr, beta1, beta2,
                    adam_eps, loss_accum=None, step_counter=None, next_mb=None):
    """hjbx_value_loss_adam_f32: params_update in one call (gradient, counts, mix, losses, Adam) for a single process; the flat gradient buffer is
    not materialised on the default path.  next_mb (next_minibatch(...)): the epilogue also assembles the minibatch of update step_counter + 1.
    -> losses (3,) = [total, hjb, termination]"""
    B = x.shape[0]
    _chk(x, "x", (B, sys.n), torch.float32)
    _chk(cost, "cost", (B,), torch.float32)
    _chk(done, "done", (B,), torch.float32)
    st = _adam_struct(params, exp_avgs, exp_avg_sqs, steps, ticket, lr, beta1, beta2, adam_eps)
    losses = torch.empty((3,), dtype=torch.float32, device=x.device)
    reg_dev, reg = _reg_args(regularization)
    if loss_accum is not None:
        _chk(loss_accum, "loss_accum", (3,), torch.float32)
    if step_counter is not None:
        _chk(step_counter, "step_counter", (1,), torch.int32)
    ws = _workspaces(x.device).grad(lib().hjbx_value_loss_adam_workspace_bytes(B))
    check(lib().hjbx_value_loss_adam_f32(sys.ptr, ref(task), ref(mlp_desc), int(mode), _p(x), _p(cost), _p(done), reg_dev, reg, float(eps), C.byref(st), _p(losses),
                                         _p(loss_accum), _p(step_counter), None if next_mb is None else C.byref(next_mb), _p(ws), B, _stream()))
    return losses


def release_workspaces(stream=None):
    """Drop the eager workspace sets (reduce tickets, rollout flags, parameter-gradient scratch) of one stream handle, or of every stream
    (`stream=None`).  They are re-created -- zero-filled where the kernels need that -- on next use.  The sets owned by captured graphs
    are not touched: they live exactly as long as their owner.  Call it when a stream goes away, or after an eager launch was aborted (a
    device fault, a killed kernel): the ticket / flag words are only guaranteed to be zero after launches that ran to completion."""
    for key in [k for k in _eager if stream is None or k[1] == stream]:
        del _eager[key]


def mix_gradients(flat, n_params, regularization, eps, loss_accum=None, step_counter=None):
    """hjbx_mix_gradients_f32: -> (mixed (P,), losses (3,) = [total, hjb, termination]).  `regularization`: float or 0-dim float32 CUDA tensor.
    loss_accum (3,) float32: the losses are added to it on the device; step_counter (1,) int32: incremented on the device."""
    _chk(flat, "flat", (2 * n_params + 4,), torch.float32)
    mixed = torch.empty((n_params,), dtype=torch.float32, device=flat.device)
    losses = torch.empty((3,), dtype=torch.float32, device=flat.device)
    if torch.is_tensor(regularization):
        _chk(regularization, "regularization", (), torch.float32)
        reg_dev, reg = _p(regularization), 0.0
    else:
        reg_dev, reg = None, float(regularization)
    if loss_accum is not None:
        _chk(loss_accum, "loss_accum", (3,), torch.float32)
    if step_counter is not None:
        _chk(step_counter, "step_counter", (1,), torch.int32)
    check(lib().hjbx_mix_gradients_f32(_p(flat), int(n_params), reg_dev, reg, float(eps), _p(mixed), _p(losses), _p(loss_accum), _p(step_counter), _stream()))
    return mixed, losses


def mix_adam(flat, regularization, eps, params, exp_avgs, exp_avg_sqs, steps, ticket, lr, beta1, beta2, adam_eps, loss_accum=None, step_counter=None):
    """hjbx_mix_adam_f32: mix of the two gradients + one Adam step on the three weight matrices, in place, one launch.  -> losses (3,)"""
    P = sum(p.numel() for p in params)
    _chk(flat, "flat", (2 * P + 4,), torch.float32)
    st = _adam_struct(params, exp_avgs, exp_avg_sqs, steps, ticket, lr, beta1, beta2, adam_eps)
    losses = torch.empty((3,), dtype=torch.float32, device=flat.device)
    reg_dev, reg = _reg_args(regularization)
    if loss_accum is not None:
        _chk(loss_accum, "loss_accum", (3,), torch.float32)
    if step_counter is not None:
        _chk(step_counter, "step_counter", (1,), torch.int32)
    check(lib().hjbx_mix_adam_f32(_p(flat), reg_dev, reg, float(eps), C.byref(st), _p(losses), _p(loss_accum), _p(step_counter), _stream()))
    return losses


def replay_gather(buf_x, buf_cost, buf_done, perm, step_counter, reg_table, xs, costs, dones, reg_out):
    """hjbx_replay_gather_f32: minibatch number step_counter[0] (read on the device) of the epoch's permutation into xs / costs / dones, and the
    regularisation weight of that update into reg_out (0-dim float32)."""
    batch, n = xs.shape
    _chk(buf_x, "buf_x", (buf_x.shape[0], n), torch.float32)
    _chk(perm, "perm", (perm.shape[0],), torch.int32)
    _chk(step_counter, "step_counter", (1,), torch.int32)
    _chk(costs, "costs", (batch,), torch.float32)
    _chk(dones, "dones", (batch,), torch.float32)
    _chk(reg_out, "reg_out", (), torch.float32)
    _chk(reg_table, "reg_table", (reg_table.shape[0],), torch.float32)
    check(lib().hjbx_replay_gather_f32(_p(buf_x), _p(buf_cost), _p(buf_done), int(buf_x.shape[0]), int(n), _p(perm), int(perm.shape[0]), _p(step_counter),
                                       _p(reg_table), int(reg_table.shape[0]), int(batch), _p(xs), _p(costs), _p(dones), _p(reg_out), _stream()))


def replay_append(traj, cost, done_step, buf_x, buf_cost, buf_done, head):
    """hjbx_replay_append_f32 / _f64: the tuples t <= done_step[b] of a time-major rollout log (traj (T+1, B, n), cost (T+1, B)) appended to the
    replay ring (buf_x (capacity, n), buf_cost, buf_done (capacity,)) whose next write slot is `head`, trajectory by trajectory, keeping the
    last `capacity` of them.  -> header, a (4,) int64 DEVICE tensor [records emitted K, records dropped, out-of-range done_step entries, 0];
    with a nonzero third entry nothing was appended.  Nothing here synchronises: the caller reads the header when it needs the counts."""
    T1, B, n = traj.shape
    capacity = buf_x.shape[0]
    _sfx(traj)
    _chk(traj, "traj", (T1, B, n))
    _chk(cost, "cost", (T1, B), traj.dtype)
    _chk(done_step, "done_step", (B,), torch.int32)
    _chk(buf_x, "buf_x", (capacity, n), traj.dtype)
    _chk(buf_cost, "buf_cost", (capacity,), traj.dtype)
    _chk(buf_done, "buf_done", (capacity,), traj.dtype)
    for t, nm in ((cost, "cost"), (done_step, "done_step"), (buf_x, "buf_x"), (buf_cost, "buf_cost"), (buf_done, "buf_done")):
        if t.device != traj.device:
            raise ValueError(f"{nm} is on {t.device}, traj on {traj.device}")
    if T1 < 1:
        raise ValueError("traj needs at least one time step")
    if B == 0:                        # (empty tensors have no address to hand over)
        return torch.zeros((4,), dtype=torch.int64, device=traj.device)
    header = torch.empty((4,), dtype=torch.int64, device=traj.device)
    ws =_workspaces(traj.device).append(lib().hjbx_replay_append_workspace_bytes(B))
    check(_fn("replay_append", traj)(_p(traj), _p(cost), _p(done_step), T1 - 1, B, n, _p(buf_x), _p(buf_cost), _p(buf_done), capacity, int(head),
                                     _p(header), _p(ws), _stream()))
    return header
