#!/usr/bin/env python3
"""Generate tests/golden/offstock.npz (+ offstock.json, the settings) from the reference's own NumPy code at the OFF-STOCK constants of
tests/offstock.py: every physical constant, control limit and cost matrix away from the values of the .gin files.

Runs where a checkout of the reference is available (--reference, or $HJB_REFERENCE); the fixture is plain data.  The reference is imported
with the placeholder `jax` / `gin` modules of tools/gen_golden.py (they implement no arithmetic).

Keys are "<system>_<ARRAY>":
  X U F1 F2 XDOT XNEXT XWRAP umin umax            48 points per system (angles over several periods, near-hover roll / pitch off tan's pole)
  M C G (cartpole, acrobot), E (acrobot)          manipulator terms
  K P Alin Blin                                   the model-based controller's set-up mathematics with the dense Q, R of tests/offstock.py
  CX CU                                           pointwise controls (every third point next to the target: both branches of the energy-shaping laws)
  XS US                                           a 60-step closed loop
and for Quadrotors2D the min-snap plan ms_*: waypoints, avg_speed, interval_t, cumulated_t, coeff, t, x_ref, u_ref, x0, traj, u, cost, K.

The reference's acrobot cannot be constructed (stale constructor: the attributes are set by hand, as tools/gen_golden.py does) and its
energy-shaping law clips to +-umax, a scalar: the law is evaluated with umax = inf and the asymmetric clip is applied here (offstock.json).
"""
import argparse
import json
import math
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
from gen_golden import _install_placeholders  # noqa: E402
import offstock as OS  # noqa: E402

NPTS = 48
LOOP = 60
STOCK_X0 = {"linear": ([0, 0], [1, 1]), "cartpole": ([0, 3.14, 0, 0], [2.4, 0.05, 1, 0.05]), "quad2d": ([0] * 6, [1] * 6),
            "nearhover": ([0] * 10, [1, 1, 1, 0.5, 0.5, 1, 1, 1, 0.5, 0.5])}
ANGLE_IDX = {"linear": [], "cartpole": [1], "acrobot": [0, 1], "quad2d": [2], "nearhover": [3, 4]}
MS_WAYPOINTS = [[0.25, -0.125], [1.0, 0.5], [1.75, -0.25], [0.5, 1.0]]
MS_SPEED = 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("HJB_REFERENCE"), required="HJB_REFERENCE" not in os.environ)
    ap.add_argument("--out", default=os.path.join(HERE, "..", "tests", "golden"))
    args = ap.parse_args()
    out = os.path.abspath(args.out)

    _install_placeholders()
    sys.path.insert(0, args.reference)
    import numpy as np
    from configs.dynamics.dynamics_config import CartpoleDynamicsConfig, LinearDynamicsConfig, NearHoverQuadcopterConfig, Quadrotors2DConfig
    from controller.acrobot_energy_shaping import AcrobotEnergyShapingController
    from controller.cartpole_energy_shaping import CartpoleEnergyShapingController
    from controller.lqr import LQR
    from controller.quadrotors_model_based_controller import (NearHoverQuadcopterHoveringController, Quadrotors2DHoveringController,
                                                              Quadrotors2DWaypointsPlanner)
    from dynamics.acrobot import Acrobot
    from dynamics.cartpole import Cartpole
    from dynamics.linear import LinearDynamics
    from dynamics.quadrotors import NearHoverQuadcopter, Quadrotors2D

    def make(name):
        if name == "acrobot":
            p = dict(OS.CONSTANTS["acrobot"], umax=np.inf, dt=OS.DT)
            a = object.__new__(Acrobot)
            a.dim, a.control_dim, a.state_dim, a.p = 2, 1, 4, p
            a.m1, a.m2, a.l1, a.l2, a.I1, a.I2 = (p[k] for k in ("m1", "m2", "l1", "l2", "I1", "I2"))
            a.g, a.dt, a.umax = p["g"], p["dt"], np.inf
            return a
        cls, cfg = {"linear": (LinearDynamics, LinearDynamicsConfig), "cartpole": (Cartpole, CartpoleDynamicsConfig),
                    "quad2d": (Quadrotors2D, Quadrotors2DConfig), "nearhover": (NearHoverQuadcopter, NearHoverQuadcopterConfig)}[name]
        kw = dict(OS.CONSTANTS[name], seed=0, dt=OS.DT, umin=OS.LIMITS[name][0], umax=OS.LIMITS[name][1], x0_mean=STOCK_X0[name][0],
                  x0_std=STOCK_X0[name][1])
        return cls(cfg(**kw))

    rng = np.random.default_rng(20261021)
    rec = {}
    dyn = {}
    for name in ("linear", "cartpole", "acrobot", "quad2d", "nearhover"):
        d = dyn[name] = make(name)
        n, m = OS.DIMS[name]
        umin, umax = (np.asarray(v, np.float64) for v in OS.LIMITS[name])
        X = rng.uniform(-1, 1, size=(NPTS, n)) * 4.0
        X[:6] *= 3.0                                                   # several periods away on the angle slots
        X[6] = 0.0
        if name == "nearhover":                                        # roll, pitch: k 2 pi + (-1.2, 1.2), cos >= 0.36
            X[:, 3:5] = rng.uniform(-1.2, 1.2, size=(NPTS, 2)) + 2 * np.pi * rng.integers(-2, 3, size=(NPTS, 2))
        mid, half = 0.5 * (umax + umin), 0.5 * (umax - umin)
        U = mid + rng.uniform(-1.5, 1.5, size=(NPTS, m)) * half        # a third beyond either limit
        F1 = np.zeros((NPTS, n)); F2 = np.zeros((NPTS, n, m)); XD = np.zeros((NPTS, n)); XN = np.zeros((NPTS, n)); XW = np.zeros((NPTS, n))
        for i in range(NPTS):
            x, u = X[i].copy(), U[i].copy()
            f1, f2 = d.get_control_affine_matrix(x)
            F1[i] = f1; F2[i] = np.asarray(f2).reshape(n, m)
            XD[i] = d.dynamics_step(x, u)
            if name == "acrobot":                                      # == Dynamics.simulate's body (the acrobot's own call site is stale)
                XN[i] = d.states_wrap(x + d.dynamics_step(x, np.clip(u, umin, umax)) * d.dt)
            else:
                XN[i] = d.simulate(x.copy(), u)
            XW[i] = d.states_wrap(x.copy())
        r = dict(X=X, U=U, F1=F1, F2=F2, XDOT=XD, XNEXT=XN, XWRAP=XW, umin=umin, umax=umax)
        if name in ("cartpole", "acrobot"):
            r["M"] = np.stack([d.get_M(x) for x in X]); r["C"] = np.stack([d.get_C(x) for x in X]); r["G"] = np.stack([d.get_G(x) for x in X])
        if name == "acrobot":
            r["E"] = np.array([d.energy(x) for x in X])
        rec.update({f"{name}_{k}": v for k, v in r.items()})

    def loop(d, law, x0, sim=None):
        xs, us = [np.array(x0, np.float64)], []
        for _ in range(LOOP):
            u = np.atleast_1d(law(xs[-1].copy())).astype(np.float64)
            us.append(u)
            xs.append(sim(xs[-1], u) if sim else d.simulate(xs[-1].copy(), u))
        return np.array(xs), np.array(us)

    notes = {}
    # ---- linear: LQR with the dense Q, R -----------------------------------------------------------------------------------------------------
    Q2, R1 = OS.dense_Q(2), OS.dense_R(1)
    lqr = LQR(dyn["linear"], Q2, R1)
    CX = rec["linear_X"] * 0.5
    xs, us = loop(dyn["linear"], lqr.get_control_efforts, [0.75, -0.5])
    rec.update(linear_K=lqr.K, linear_P=lqr.P, linear_CX=CX, linear_CU=np.stack([np.atleast_1d(lqr.get_control_efforts(x.copy())) for x in CX]),
               linear_XS=xs, linear_US=us)

    # ---- cart-pole energy shaping ------------------------------------------------------------------------------------------------------------
    Q4 = OS.dense_Q(4)
    ces = CartpoleEnergyShapingController(dyn["cartpole"], Q=Q4, R=R1)
    K, P = ces.get_lqr_term()
    A_, B_ = ces.get_linearized_dynamics()
    CX = rec["cartpole_X"].copy()
    CX[::3, 1] = np.pi + 0.05 * rng.standard_normal(CX[::3, 1].shape)          # next to the upright: the LQR branch
    CX[::3, 3] = 0.1 * rng.standard_normal(CX[::3, 3].shape)
    CU = np.stack([np.atleast_1d(ces.get_control_efforts(x.copy())) for x in CX])
    lqr_branch = np.array([abs(ces.energy(x) - ces.energy(ces.xf)) < 1 and np.linalg.norm(dyn["cartpole"].states_wrap(x - ces.xf)[[1, 3]]) < 1 for x in CX])
    assert 4 <= lqr_branch.sum() <= NPTS - 4, lqr_branch.sum()
    xs, us = loop(dyn["cartpole"], ces.get_control_efforts, [0.5, 2.0, 0.25, -0.5])
    rec.update(cartpole_K=K, cartpole_P=P, cartpole_Alin=A_, cartpole_Blin=B_, cartpole_Kes=np.asarray(ces.K, np.float64), cartpole_CX=CX,
               cartpole_CU=CU, cartpole_CBRANCH=lqr_branch, cartpole_XS=xs, cartpole_US=us)

    # ---- acrobot energy shaping (law with umax = inf, asymmetric clip applied here) -------------------------------------------------------------
    ac = dyn["acrobot"]
    a_umin, a_umax = (np.asarray(v, np.float64) for v in OS.LIMITS["acrobot"])
    aes0 = AcrobotEnergyShapingController(ac, Q=Q4, R=R1)
    K, P = aes0.get_lqr_term()
    A_, B_ = aes0.get_linearized_dynamics()
    CX = rec["acrobot_X"].copy()
    CX[::3, 0] = np.pi + 0.05 * rng.standard_normal(CX[::3, 0].shape)
    CX[::3, 1:] = 0.05 * rng.standard_normal(CX[::3, 1:].shape)
    dx = np.array([np.hstack([(x - aes0.xf)[:2] + np.pi, (x - aes0.xf)[2:]]) for x in CX])
    dx[:, :2] = dx[:, :2] % (2 * np.pi) - np.pi
    quad_form = np.einsum("bi,ij,bj->b", dx, P, dx)
    eps = 2.0 ** round(math.log2(np.median(quad_form)))                        # a region that splits the points between the two branches
    aes = AcrobotEnergyShapingController(ac, Q=Q4, R=R1, eps=eps)
    inside = quad_form < eps
    assert 4 <= inside.sum() <= NPTS - 4 and np.abs(quad_form / eps - 1).min() > 1e-3, (inside.sum(), np.abs(quad_form / eps - 1).min())
    law = lambda x: np.clip(np.atleast_1d(aes.get_control_efforts(x)), a_umin, a_umax)
    ac_sim = lambda x, u: ac.states_wrap(x + ac.dynamics_step(x, np.clip(u, a_umin, a_umax)) * ac.dt)
    xs, us = loop(ac, law, [2.5, 0.5, 0.25, -0.5], sim=ac_sim)
    rec.update(acrobot_K=K, acrobot_P=P, acrobot_Alin=A_, acrobot_Blin=B_, acrobot_Kes=np.asarray(aes.K, np.float64), acrobot_eps=np.float64(eps),
               acrobot_CX=CX, acrobot_CU=np.stack([law(x.copy()) for x in CX]), acrobot_CBRANCH=inside, acrobot_XS=xs, acrobot_US=us)
    notes["acrobot"] = ("reference Acrobot() cannot be constructed (stale constructor): attributes set by hand; its energy-shaping law clips to a "
                        "scalar +-umax: evaluated with umax = inf, the asymmetric clip applied by the generator")

    # ---- hover LQRs ----------------------------------------------------------------------------------------------------------------------------
    for name, cls, xf in (("quad2d", Quadrotors2DHoveringController, [0.5, -0.25, 0, 0, 0, 0]),
                          ("nearhover", NearHoverQuadcopterHoveringController, [0.25, -0.5, 0.375, 0, 0, 0, 0, 0, 0, 0])):
        n, m = OS.DIMS[name]
        c = cls(dyn[name], np.array(xf, np.float64), OS.dense_Q(n), OS.dense_R(m))
        CX = rec[f"{name}_X"] * (0.25 if name == "nearhover" else 1.0)
        x0 = np.array(xf, np.float64) + 0.3 * rng.uniform(-1, 1, n)
        xs, us = loop(dyn[name], c.get_control_efforts, x0)
        rec.update({f"{name}_K": c.K, f"{name}_P": c.P, f"{name}_Alin": c.A, f"{name}_Blin": c.B, f"{name}_ctrl_xf": np.array(xf, np.float64),
                    f"{name}_ctrl_uf": np.asarray(c.uf, np.float64), f"{name}_CX": CX,
                    f"{name}_CU": np.stack([c.get_control_efforts(x.copy()) for x in CX]), f"{name}_XS": xs, f"{name}_US": us})

    # ---- min-snap plan and a tracking loop (tools/gen_golden_minsnap.py, at the off-stock m, r, I, g, box) --------------------------------------
    quad = dyn["quad2d"]
    wp = np.asarray(MS_WAYPOINTS, np.float64)
    planner = Quadrotors2DWaypointsPlanner(wp, quad, avg_speed=MS_SPEED)
    dt = float(quad.dt)
    steps = int(math.ceil(planner.cumulated_t[-1] / dt)) + 6
    t = np.array([k * dt for k in range(steps)], np.float64)
    gap = np.abs(t[:, None] - planner.cumulated_t[None, 1:]).min()
    assert gap >= 1e-3, gap                                                    # a float32 time picks the same segment
    ref = [planner.update(tk) for tk in t]
    x_ref = np.array([r[0] for r in ref], np.float64); u_ref = np.array([r[1] for r in ref], np.float64)
    Kq = np.asarray(rec["quad2d_K"], np.float64)
    Q6, R2 = OS.dense_Q(6), OS.dense_R(2)
    umin, umax = (np.asarray(v, np.float64) for v in OS.LIMITS["quad2d"])
    x0 = np.zeros((4, 6)); x0[:, :2] = wp[0]; x0 += rng.uniform(-0.3, 0.3, size=(4, 6))
    traj = np.zeros((4, steps + 1, 6)); us = np.zeros((4, steps, 2)); cost = np.zeros((4, steps))
    for b in range(4):
        x = x0[b].copy(); traj[b, 0] = x
        for k in range(steps):
            xr, ur = planner.update(t[k])
            e = quad.states_wrap(x - xr)
            u = np.clip(ur - Kq @ e, umin, umax)
            cost[b, k] = (e @ Q6 @ e + (u - ur) @ R2 @ (u - ur)) * dt
            x = quad.simulate(x, u)
            us[b, k] = u; traj[b, k + 1] = x
    rec.update(ms_waypoints=wp, ms_avg_speed=np.float64(MS_SPEED), ms_interval_t=planner.interval_t, ms_cumulated_t=planner.cumulated_t,
               ms_coeff=planner.coeff, ms_t=t, ms_x_ref=x_ref, ms_u_ref=u_ref, ms_x0=x0, ms_traj=traj, ms_u=us, ms_cost=cost, ms_K=Kq, ms_Q=Q6,
               ms_R=R2, ms_umin=umin, ms_umax=umax, ms_params=np.array([quad.m, quad.r, quad.I, quad.g], np.float64), ms_dt=np.float64(dt))
    print(f"min-snap: {steps} steps, boundary gap {gap:.2e} s, clipped controls {int(((us == umin) | (us == umax)).sum())} of {us.size}, "
          f"max |u_ref| {np.abs(u_ref).max():.3f}")

    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "offstock.npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in rec.items()})
    settings = dict(dt=OS.DT, constants=OS.CONSTANTS, limits={k: dict(umin=v[0], umax=v[1]) for k, v in OS.LIMITS.items()},
                    Q={str(n): OS.dense_Q(n).tolist() for n in (2, 4, 6, 10)}, R={str(m): OS.dense_R(m).tolist() for m in (1, 2, 3)},
                    points=NPTS, loop_steps=LOOP, minsnap=dict(waypoints=MS_WAYPOINTS, avg_speed=MS_SPEED), acrobot_eps=float(eps), notes=notes,
                    note="generated by tools/gen_golden_offstock.py from the reference's NumPy branch")
    with open(os.path.join(out, "offstock.json"), "w") as f:
        json.dump(settings, f, indent=1, sort_keys=True)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
