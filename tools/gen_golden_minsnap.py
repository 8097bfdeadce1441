#!/usr/bin/env python3
"""Generate tests/golden/minsnap_quad2d.npz from the reference's own NumPy code: the min-snap waypoint planner
(controller/quadrotors_model_based_controller.py:77-233) and a tracking closed loop composed of reference pieces only.

Runs where a checkout of the reference is available (--reference, or $HJB_REFERENCE); the fixture it writes is plain data and is what the
tests read.  The reference is imported with the placeholder `jax` / `gin` modules of tools/gen_golden.py (they implement no arithmetic:
the reference's NumPy branches never call into them).

Per plan i = 0..3 the fixture holds
  p{i}_waypoints (P, 2), p{i}_avg_speed, p{i}_interval_t (S,), p{i}_cumulated_t (P,), p{i}_coeff (2, S, 8)   planner attributes
  p{i}_t (K,)                 the grid t_k = t0 + k dt, k = 0 .. ceil(T_plan / dt) + 9 (computed so, never accumulated)
  p{i}_x_ref (K, 6), p{i}_u_ref (K, 2)                                                                        planner.update(t_k)
  p{i}_x0 (4, 6), p{i}_traj (4, K + 1, 6), p{i}_u (4, K, 2), p{i}_cost (4, K)                                 tracking closed loop
and once: K (2, 6) hover-LQR gain for Q = I6, R = I2, Q, R, umin, umax, dt, t0, params = [m, r, I, g].
The closed loop is   u_k = clip(u_ref(t_k) - K wrap(x_k - x_ref(t_k)), umin, umax),  x_{k+1} = Quadrotors2D.simulate(x_k, u_k),
cost_k = (e'Qe + (u_k - u_ref)'R(u_k - u_ref)) dt.

Usage:  python tools/gen_golden_minsnap.py --reference /path/to/reference [--out tests/golden]
"""
import argparse
import math
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import _install_placeholders  # noqa: E402

W0 = [[0.0, 0.0], [1.0, 0.5], [1.5, -0.5], [0.0, 1.0]]
PLANS = [(W0, 1.0), (W0, 0.25), ([[0.0, 0.0], [1.0, 1.0]], 1.0), ([[0.2, -0.1], [1.0, 0.6], [1.9, 0.1], [2.6, 0.9]], 1.0)]
QUAD2D_GIN = dict(seed=0, m=1, r=0.25, g=9.81, I=0.0625, dt=0.05, x0_mean=[0] * 6, x0_std=[1] * 6, umin=[-20, -20], umax=[20, 20])
T0 = 0.0
MIN_BOUNDARY_DISTANCE = 1e-3   # seconds between any grid time and a segment boundary: a float32 time must pick the same segment


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("HJB_REFERENCE"), required="HJB_REFERENCE" not in os.environ)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "tests", "golden"))
    args = ap.parse_args()
    out = os.path.abspath(args.out)

    _install_placeholders()
    sys.path.insert(0, args.reference)
    import numpy as np
    from configs.dynamics.dynamics_config import Quadrotors2DConfig
    from dynamics.quadrotors import Quadrotors2D
    from controller.quadrotors_model_based_controller import Quadrotors2DHoveringController, Quadrotors2DWaypointsPlanner

    quad = Quadrotors2D(Quadrotors2DConfig(**QUAD2D_GIN))
    Q, R = np.eye(6), np.eye(2)
    hover = Quadrotors2DHoveringController(quad, np.zeros(6), Q, R)
    K = np.asarray(hover.K, np.float64)
    umin, umax = (np.asarray(v, np.float64) for v in quad.get_control_limit())
    dt = float(quad.dt)
    rec = dict(K=K, Q=Q, R=R, umin=umin, umax=umax, dt=np.float64(dt), t0=np.float64(T0),
               params=np.array([quad.m, quad.r, quad.I, quad.g], np.float64), n_plans=np.int64(len(PLANS)))
    rng = np.random.default_rng(20261020)
    for i, (wp, speed) in enumerate(PLANS):
        wp = np.asarray(wp, np.float64)
        planner = Quadrotors2DWaypointsPlanner(wp, quad, avg_speed=speed)
        steps = int(math.ceil(planner.cumulated_t[-1] / dt)) + 10
        t = np.array([T0 + k * dt for k in range(steps)], np.float64)
        gap = np.abs(t[:, None] - planner.cumulated_t[None, 1:]).min()
        assert gap >= MIN_BOUNDARY_DISTANCE, (i, gap)
        ref = [planner.update(tk) for tk in t]
        x_ref = np.array([r[0] for r in ref], np.float64)
        u_ref = np.array([r[1] for r in ref], np.float64)
        x0 = np.zeros((4, 6))
        x0[:, :2] = wp[0]
        x0 += rng.uniform(-0.3, 0.3, size=(4, 6))
        traj = np.zeros((4, steps + 1, 6)); us = np.zeros((4, steps, 2)); cost = np.zeros((4, steps))
        for b in range(4):
            x = x0[b].copy()
            traj[b, 0] = x
            for k in range(steps):
                xr, ur = planner.update(t[k])
                e = quad.states_wrap(x - xr)
                u = np.clip(ur - K @ e, umin, umax)
                cost[b, k] = (e @ Q @ e + (u - ur) @ R @ (u - ur)) * dt
                x = quad.simulate(x, u)
                us[b, k] = u
                traj[b, k + 1] = x
        print(f"plan {i}: S = {wp.shape[0] - 1}, T_plan = {planner.cumulated_t[-1]:.4f} s, {steps} steps, boundary gap {gap:.2e} s, "
              f"max |u| {np.abs(us).max():.3f}, final tracking error {np.abs(quad.states_wrap(traj[:, -1] - x_ref[-1])).max():.2e}")
        rec.update({f"p{i}_waypoints": wp, f"p{i}_avg_speed": np.float64(speed), f"p{i}_interval_t": planner.interval_t,
                    f"p{i}_cumulated_t": planner.cumulated_t, f"p{i}_coeff": planner.coeff, f"p{i}_t": t, f"p{i}_x_ref": x_ref,
                    f"p{i}_u_ref": u_ref, f"p{i}_x0": x0, f"p{i}_traj": traj, f"p{i}_u": us, f"p{i}_cost": cost})
    path = os.path.join(out, "minsnap_quad2d.npz")
    np.savez(path, **rec)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
