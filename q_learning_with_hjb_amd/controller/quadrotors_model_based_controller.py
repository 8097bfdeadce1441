"""Model-based controllers of the quadrotors (reference controller/quadrotors_model_based_controller.py).

Hover LQR for Quadrotors2D and NearHoverQuadcopter: u = clip(-K wrap(x - xf) + uf)  (:7-38 and :40-75).
Quadrotors2DWaypointsPlanner (:77-233): a 7th-order minimum-snap polynomial through waypoints, the differential-flatness map to the full
state and the two rotor thrusts, and update(t).  The plan is solved on the host in float64 NumPy; `reference()` evaluates it on the device
(hjbx_minsnap_reference_*), and Quadrotors2DTrackingController closes the loop u = clip(u_ref(t) - K wrap(x - x_ref(t))) around it in one
kernel launch (hjbx_rollout_minsnap_tracking_*)."""
import numpy as np
import scipy.linalg

import torch

from .. import _abi, _ops
from ..dynamics.dynamics_basic import _from_device, _to_device
from .feedback import DeviceFeedbackController


class _HoverLQR(DeviceFeedbackController):
    def _finish(self):
        self.P = scipy.linalg.solve_continuous_are(self.A, self.B, self.Q, self.R)
        self.K = np.dot(scipy.linalg.inv(self.R), np.dot(self.B.T, self.P))

    def _descriptor(self):
        n, m = self.dynamics.get_dimension()
        return _abi.make_controller(_abi.CTRL_LINEAR_FEEDBACK, n, m, self.K, xf=self.xf, uf=self.uf, wrap_error=True)


class Quadrotors2DHoveringController(_HoverLQR):
    def __init__(self, dynamics, xf: np.ndarray, Q: np.ndarray, R: np.ndarray) -> None:
        super().__init__()
        self.dynamics, self.xf, self.Q, self.R = dynamics, np.asarray(xf), np.asarray(Q), np.asarray(R)
        self.umin, self.umax = self.dynamics.get_control_limit()
        if np.linalg.norm(self.xf[2:]) > 0:
            raise ValueError("Final Velocity or Angle is not zero")
        d = self.dynamics
        self.uf = d.m * d.g / 2 * np.ones(2)
        self.A = np.vstack([np.hstack([np.zeros((3, 3)), np.eye(3)]), np.array([0, 0, -d.g, 0, 0, 0]), np.zeros((2, 6))])
        self.B = np.vstack([np.zeros((4, 2)), np.ones((1, 2)) / d.m, np.array([d.r / d.I, -d.r / d.I])])
        self._finish()


class NearHoverQuadcopterHoveringController(_HoverLQR):
    def __init__(self, dynamics, xf: np.ndarray, Q: np.ndarray, R: np.ndarray) -> None:
        super().__init__()
        self.dynamics, self.xf, self.Q, self.R = dynamics, np.asarray(xf), np.asarray(Q), np.asarray(R)
        self.umin, self.umax = self.dynamics.get_control_limit()
        if np.linalg.norm(self.xf[3:]) > 0:
            raise ValueError("Final Velocity or Angle is not zero")
        d = self.dynamics
        self.uf = np.array([d.g * d.m / d.kT, 0, 0])
        self.A = np.vstack([np.hstack([np.zeros((5, 5)), np.eye(5)]),
                            np.array([0, 0, 0, d.g, 0, 0, 0, 0, 0, 0]),
                            np.array([0, 0, 0, 0, d.g, 0, 0, 0, 0, 0]),
                            np.zeros((3, 10))])
        self.B = np.vstack([np.zeros((7, 3)), np.array([d.kT / d.m, 0, 0]), np.array([0, d.n0, 0]), np.array([0, 0, d.n0])])
        self._finish()


class Quadrotors2DWaypointsPlanner:
    """Minimum-snap trajectory through `waypoints` (P, 2) -- or (P, 3): coefficients only -- with segment i lasting distance_i / avg_speed.

    Attributes as upstream: points, points_num, interval_t (S,), cumulated_t (P,), coeff (dim, S, 8) with S = P - 1, ascending powers of the
    time since the segment began.  `waypoints` may also be (Bp, P, dim): Bp plans of the same length, one per environment; every attribute
    then has a leading Bp axis (coeff (Bp, dim, S, 8)) and the linear systems are solved stacked.  Everything here is float64 NumPy and needs
    no GPU, except `reference()`."""

    def __init__(self, waypoints: np.ndarray, dynamics, avg_speed=0.25) -> None:
        pts = np.asarray(waypoints, dtype=np.float64)
        if pts.ndim not in (2, 3) or pts.shape[-1] not in (2, 3):
            raise ValueError("The waypoints dim should either be 2D or 3D")
        if pts.shape[-2] < 2:
            raise ValueError("a plan needs at least two waypoints")
        if not avg_speed > 0:
            raise ValueError(f"avg_speed must be positive, got {avg_speed}")
        self.stacked = pts.ndim == 3
        self.dim = pts.shape[-1]
        self.points = pts
        self.dynamics = dynamics
        self.points_num = pts.shape[-2]
        self.avg_speed = avg_speed
        self.displacements = np.diff(pts, axis=-2)
        self.distants = np.sqrt(np.sum(self.displacements ** 2, axis=-1))
        self.interval_t = self.distants / self.avg_speed
        self.cumulated_t = np.concatenate([np.zeros(pts.shape[:-2] + (1,)), np.cumsum(self.interval_t, axis=-1)], axis=-1)
        self.coeff = self.solve_minimum_snap_coefficient()
        self._device_plans = {}

    # -- the linear system -------------------------------------------------------------------------
    def get_polynomial_term(self, t, n, order=7) -> np.ndarray:
        """z with d^n/dt^n sum_i c_i t^i = c . z:  z_i = i! / (i - n)! t^(i - n) for i >= n, else 0."""
        i = np.arange(order + 1)
        falling = np.ones(order + 1)
        for j in range(n):
            falling = falling * (i - j)
        return np.where(i >= n, falling * np.float64(t) ** np.maximum(i - n, 0), 0.0)

    def _system(self, interval_t, points):
        """A (8S, 8S) and b (dim, 8S) of ONE plan: rest-to-rest end conditions (position, and zero velocity, acceleration and jerk at both
        ends), both neighbours through every interior waypoint, derivatives 1..6 continuous there."""
        S, z = self.points_num - 1, self.get_polynomial_term
        A = np.zeros((8 * S, 8 * S))
        b = np.zeros((self.dim, 8 * S))
        first, last = slice(0, 8), slice(8 * (S - 1), 8 * S)
        for n in range(4):
            A[2 * n, first] = z(0.0, n)
            A[2 * n + 1, last] = z(interval_t[-1], n)
        b[:, 0], b[:, 1] = points[0], points[-1]
        row = 8
        for i in range(S - 1):               # the interior waypoint between segments i and i + 1
            A[row, 8 * i:8 * i + 8] = z(interval_t[i], 0)
            A[row + 1, 8 * i + 8:8 * i + 16] = z(0.0, 0)
            b[:, row] = b[:, row + 1] = points[i + 1]
            row += 2
        for i in range(S - 1):
            for n in range(1, 7):
                A[row, 8 * i:8 * i + 8] = z(interval_t[i], n)
                A[row, 8 * i + 8:8 * i + 16] = -z(0.0, n)
                row += 1
        return A, b

    def solve_minimum_snap_coefficient(self) -> np.ndarray:
        """coeff (dim, S, 8), or (Bp, dim, S, 8) from one stacked np.linalg.solve."""
        S = self.points_num - 1
        if not self.stacked:
            A, b = self._system(self.interval_t, self.points)
            return np.linalg.solve(A, b.T).T.reshape(self.dim, S, 8)
        systems = [self._system(it, pts) for it, pts in zip(self.interval_t, self.points)]
        A = np.stack([a for a, _ in systems])
        b = np.stack([b.T for _, b in systems])
        return np.swapaxes(np.linalg.solve(A, b), -1, -2).reshape(-1, self.dim, S, 8)

    # -- update(t) on the host ------------------------------------------------------------------------
    def flat_output_to_full_states_and_inputs_2D(self, t, coeff):
        """([x, y, theta, x_dot, y_dot, theta_dot], [u_1, u_2]) of the flat output sum_i coeff[:, i] t^i.  theta_ddot keeps upstream's
        expression, which is not the exact second derivative of theta."""
        d = self.dynamics
        order = coeff.shape[1] - 1
        der = [coeff @ self.get_polynomial_term(t, n, order) for n in range(5)]
        (x, y), (xd, yd), (x2, y2), (x3, y3), (x4, y4) = der
        den = y2 + d.g
        q = 1 + (x2 / den) ** 2
        w = x3 / den - x2 * y3 / den ** 2
        theta = -np.arctan2(x2, den)
        theta_dot = -1 / q * w
        theta_ddot = 2 * x2 / den / q ** 2 * w ** 2 - 1 / q * (x4 / den - x3 * y3 / den ** 2 - x3 * y3 / den ** 2 - x2 * y4 / den ** 2
                                                                 + 2 * x2 * y3 / den ** 3)
        torque = d.I / d.r * theta_ddot
        if np.sin(theta) != 0:
            lift = -(d.m / np.sin(theta) * x2)
        else:                                   # the hover tail, and wherever x_ddot is exactly 0
            lift = d.m / np.cos(theta) * den
        return np.array([x, y, theta, xd, yd, theta_dot]), np.array([(torque + lift) / 2, (-torque + lift) / 2])

    def _update_one(self, t, cumulated_t, coeff, end_point):
        index = int(np.nonzero(t >= cumulated_t)[0][-1])
        if index == self.points_num - 1:        # past the last waypoint: hover there
            t_local, c = 0.0, np.zeros((self.dim, coeff.shape[-1]))
            c[:, 0] = end_point
        else:
            t_local, c = t - cumulated_t[index], coeff[:, index, :]
        if self.dim != 2:
            raise NotImplementedError
        return self.flat_output_to_full_states_and_inputs_2D(t_local, c)

    def update(self, t):
        """(full_state (6,), u (2,)) of the plan at time t >= 0; (Bp, 6), (Bp, 2) for stacked plans."""
        if not self.stacked:
            return self._update_one(t, self.cumulated_t, self.coeff, self.points[-1])
        out = [self._update_one(t, ct, c, p[-1]) for ct, c, p in zip(self.cumulated_t, self.coeff, self.points)]
        return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])

    # -- the device ---------------------------------------------------------------------------------
    def device_plan(self, dtype, device):
        """(coeff (Bp, 2, S, 8) of `dtype`, cum_t (Bp, S + 1) float64, end_pt (Bp, 2)) on `device`, Bp = 1 for a single plan."""
        if self.dim != 2:
            raise NotImplementedError
        key = (dtype, str(device))
        if key not in self._device_plans:
            S = self.points_num - 1
            up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(device=device, dtype=dt).contiguous()
            self._device_plans[key] = (up(self.coeff.reshape(-1, 2, S, 8), dtype), up(self.cumulated_t.reshape(-1, S + 1), torch.float64),
                                       up(self.points.reshape(-1, S + 1, 2)[:, -1], dtype))
        return self._device_plans[key]

    def reference(self, steps, t0=0.0, dtype=torch.float32, device=None):
        """update(t0 + k dt) for k < steps on the device: time-major x_ref (steps, Bp, 6), u_ref (steps, Bp, 2) tensors of `dtype`."""
        device = _ops.require_device() if device is None else torch.device(device)
        return _ops.minsnap_reference(self.dynamics.system, *self.device_plan(dtype, device), int(steps), t0=t0)


class Quadrotors2DTrackingController(DeviceFeedbackController):
    """u = clip(u_ref(t) - K wrap(x - x_ref(t)), umin, umax) along a Quadrotors2DWaypointsPlanner; K is the gain of
    Quadrotors2DHoveringController(dynamics, 0, Q, R) (the linearisation about hover does not depend on where the hover is)."""

    def __init__(self, dynamics, planner: Quadrotors2DWaypointsPlanner, Q: np.ndarray, R: np.ndarray) -> None:
        super().__init__()
        hover = Quadrotors2DHoveringController(dynamics, np.zeros(6), Q, R)
        self.dynamics, self.planner = dynamics, planner
        self.Q, self.R, self.P, self.K = hover.Q, hover.R, hover.P, hover.K
        self.umin, self.umax = hover.umin, hover.umax

    def _descriptor(self):
        return _abi.make_controller(_abi.CTRL_LINEAR_FEEDBACK, 6, 2, self.K, wrap_error=True)

    def _task(self):
        return _abi.make_task(6, 2, self.Q, self.R, None, np.zeros(6), np.zeros(2), None, None, 0.0)

    def _run(self, x0, steps, t0, **logs):
        return _ops.rollout_minsnap_tracking(self.dynamics.system, self._descriptor(), *self.planner.device_plan(x0.dtype, x0.device), x0, int(steps),
                                             t0=t0, integrator=self.dynamics.integrator, **logs)

    def get_control_efforts(self, x, t=0.0):
        """u (2,) or (B, 2) of the tracking law at time t for x (6,) or (B, 6); numpy or torch like the Dynamics methods."""
        xt, one, kind = _to_device(x)
        return _from_device(self._run(xt, 1, t, log_traj=False, log_u=True)["u"][0], one, kind)

    def rollout(self, x0, steps, t0=0.0, log_traj=True, log_u=True, log_cost=False, log_reference=False):
        """The closed loop for `steps` steps from time t0, fused in one kernel.  x0: (B, 6) or (6,); stacked plans need B plans.  Returns a
        dict like DeviceFeedbackController.rollout: time-major `traj` (steps+1, B, 6), `u` (steps, B, 2), `total_cost`, `x_final`, optional
        `cost` (steps, B) = (e'Qe + (u-u_ref)'R(u-u_ref)) dt, and `x_ref`, `u_ref` with log_reference; numpy in -> numpy out."""
        xt, one, kind = _to_device(x0)
        out = self._run(xt, steps, t0, task=self._task(), log_traj=log_traj, log_u=log_u, log_cost=log_cost, log_reference=log_reference)
        if kind == "cuda":
            return out
        return {k: (None if v is None else (v.cpu().numpy() if kind == "numpy" else v.cpu())) for k, v in out.items()}
