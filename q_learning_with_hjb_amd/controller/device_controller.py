"""`DeviceController` -- the open half of plugin surface #2 (the reference's controller/controller_basic.py:1-5: anything with
`get_control_efforts(x)` drives a system): a control law written by the user, compiled at run time into the library's closed-loop rollout
kernel for one system (hjbx_user_controller_create, include/hjbx.h).  A swing-up law for one's own pendulum, a gain-scheduled or
time-varying law, a feed-forward term: the whole closed loop still runs in ONE kernel launch, on a built-in or a user-defined system."""
from __future__ import annotations

from .. import _abi, _ops
from ..dynamics.dynamics_basic import Dynamics, _from_device, _to_device
from .controller_basic import Controller


class DeviceController(Controller):
    """Base of user-defined control laws that run on the device.

    A subclass defines `device_source()` -> dict(source=<device code>, params=[...], env_params=0, reached=False):

    * `source`: member functions of `template <typename T, typename S> struct UserLaw { T q[len(params)]; ... }` -- the required
      `HJBX_DEV void control(const S& sys, const Limits<T, S::M>& lim, const T* x, const T* w, T t, T* u) const` writes the RAW control
      (the library clips it to the system's limits), and with `reached=True` also
      `HJBX_DEV bool reached(const S& sys, const T* x, const T* w, T t) const`, the stop test of `rollout(stop_at_target=True)`.
      The exact contract is at the top of csrc/hjbx_user_controller_kernels.hpp.
    * `params`: the values of q, shared by all environments; `set_params` replaces them without a recompile.
    * `env_params`: how many values w[0..) each environment gets from the `env_params` argument of the calls, a (B, env_params) array.

    The law is compiled at the first use, for the system of `dynamics` (built-in or user-defined), float32 and float64."""

    dynamics: Dynamics

    def __init__(self, dynamics: Dynamics) -> None:
        super().__init__()
        self.dynamics = dynamics
        self._handle = None

    def device_source(self):
        raise NotImplementedError(f"{type(self).__name__} has no control law: a DeviceController subclass defines device_source() "
                                  "(see DeviceController)")

    @property
    def handle(self) -> _abi.UserControllerHandle:
        """the compiled law (hjbx_user_controller*), built at the first use"""
        if self._handle is None:
            src = self.device_source()
            self._handle = _abi.UserControllerHandle(self.dynamics.system, src["source"], src.get("params", ()), int(src.get("env_params", 0)),
                                                     bool(src.get("reached", False)))
        return self._handle

    def set_params(self, q):
        """new values of the law's parameters q (as many as device_source() gave): no recompile, the next call uses them"""
        self.handle.set_params(q)

    def code_object(self) -> bytes:
        """the gfx950 ELF of this (system, law) pair: the six hjbx_uc_* kernels"""
        return self.handle.code_object()

    def _env_params(self, env_params, x_t):
        if env_params is None:
            return None
        w, _, _ = _to_device(env_params, like_dtype=x_t.dtype)
        if w.shape[0] == 1 and x_t.shape[0] != 1:
            w = w.expand(x_t.shape[0], w.shape[1])
        return w.contiguous()

    def get_control_efforts(self, x, t=0.0, env_params=None):
        """u (m,) or (B, m) for x (n,) or (B, n) at time t; numpy or torch like the Dynamics methods."""
        handle = self.handle                             # (a missing or broken law is reported before anything touches the device)
        xt, one, kind = _to_device(x)
        u = _ops.user_controller_eval(handle, xt, float(t), self._env_params(env_params, xt))
        return _from_device(u, one, kind)

    def _device_rollout(self, x0, steps, **kw):
        """the rollout on device tensors (x0 (B, n) on the device) -> dict of device tensors; what VHJBController.warm_start calls"""
        return _ops.user_controller_rollout(self.handle, x0, int(steps), integrator=self.dynamics.integrator, **kw)

    def rollout(self, x0, steps, task=None, terminate=False, log_traj=True, log_u=True, log_cost=False, stop_at_target=False, t0=0.0,
                env_params=None):
        """Closed loop `for k: u = self(x, t0 + k dt); x = simulate(x, u)` for `steps` steps, fused in one kernel.

        The return contract of DeviceFeedbackController.rollout: x0 (B, n) (or (n,)) -> a dict with time-major `traj` (steps+1, B, n),
        `u` (steps, B, m), optional `cost`, `total_cost`, `done_step`, `x_final`; numpy in -> numpy out.  `stop_at_target` ends an
        environment once the law's `reached` says so (`done_step` = that step index)."""
        handle = self.handle
        if stop_at_target and not handle.reached:
            raise ValueError(f"{type(self).__name__}: stop_at_target=True needs a law that defines `reached` (device_source(): reached=True)")
        t, one, kind = _to_device(x0)
        out = self._device_rollout(t, steps, task=task, terminate=terminate, log_traj=log_traj, log_u=log_u, log_cost=log_cost,
                                   stop_at_target=stop_at_target, t0=float(t0), w=self._env_params(env_params, t))
        if kind == "cuda":
            return out
        return {k: (None if v is None else (v.cpu().numpy() if kind == "numpy" else v.cpu())) for k, v in out.items()}
