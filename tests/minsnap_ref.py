"""Independent NumPy restatement of the min-snap waypoint planner and the tracking closed loop of Quadrotors2D (reference
controller/quadrotors_model_based_controller.py:77-233, dynamics/quadrotors.py:17-70, dynamics_basic.py:107-122), parametrised by dtype.

A helper like tests/hessref.py: not a test module.  It shares no code with the package.  In float64 it is pinned against the golden fixture
(tests/test_minsnap_host.py); in float32 -- every operation rounded to float32, in the reference's order, Horner's rule for the polynomials
-- it is the yardstick of the float32 kernels: what a float32 implementation of the reference achieves.  Times are
float64 in both: t_k = t0 + k dt, the segment search and the local time t - cumulated_t[i], which alone is rounded to the dtype."""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "minsnap_quad2d.npz")


def scale(a):
    """component scale of a golden array (..., n): max |a| over everything but the last axis (0.4 - 1.8 for the states, ~7 for the thrusts)"""
    a = np.asarray(a)
    return np.abs(a).reshape(-1, a.shape[-1]).max(axis=0)


def golden():
    return dict(np.load(GOLDEN))


def plan_of(g, i):
    """plan i of the fixture as a dict"""
    return {k: g[f"p{i}_{k}"] for k in ("waypoints", "avg_speed", "interval_t", "cumulated_t", "coeff", "t", "x_ref", "u_ref", "x0", "traj", "u", "cost")}


# ---- the coefficient system ----------------------------------------------------------------------------------------------------------------
def basis(t, n):
    """row z with p^(n)(t) = c . z for p = sum_i c_i t^i, i < 8"""
    z = np.zeros(8)
    for i in range(n, 8):
        z[i] = math.factorial(i) // math.factorial(i - n) * t ** (i - n)
    return z


def assemble(waypoints, avg_speed):
    """-> interval_t (S,), cumulated_t (S + 1,), A (8S, 8S), b (8S, dim) of the min-snap problem: rest to rest (zero velocity, acceleration
    and jerk at both ends), each interior waypoint met by both neighbouring segments, derivatives 1..6 continuous across it."""
    w = np.asarray(waypoints, np.float64)
    S, dim = w.shape[0] - 1, w.shape[1]
    T = np.linalg.norm(w[1:] - w[:-1], axis=1) / avg_speed
    cum = np.concatenate([[0.0], np.cumsum(T)])
    rows, rhs = [], []

    def add(seg_terms, value):
        r = np.zeros(8 * S)
        for s, z in seg_terms:
            r[8 * s:8 * s + 8] += z
        rows.append(r)
        rhs.append(np.broadcast_to(value, (dim,)).astype(np.float64))

    for n in range(4):
        add([(0, basis(0.0, n))], w[0] if n == 0 else 0.0)
        add([(S - 1, basis(T[-1], n))], w[-1] if n == 0 else 0.0)
    for s in range(S - 1):
        add([(s, basis(T[s], 0))], w[s + 1])
        add([(s + 1, basis(0.0, 0))], w[s + 1])
    for s in range(S - 1):
        for n in range(1, 7):
            add([(s, basis(T[s], n)), (s + 1, -basis(0.0, n))], 0.0)
    return T, cum, np.array(rows), np.array(rhs)


def solve(waypoints, avg_speed):
    """-> interval_t, cumulated_t, coeff (dim, S, 8), cond(A)"""
    T, cum, A, b = assemble(waypoints, avg_speed)
    c = np.linalg.solve(A, b)
    return T, cum, c.T.reshape(b.shape[1], -1, 8), np.linalg.cond(A)


# ---- update(t) ------------------------------------------------------------------------------------------------------------------------------
def _horner(c, tau, n, dt):
    """n-th derivative of sum_i c_i tau^i in dtype dt"""
    fall = lambda i: dt(math.factorial(i) // math.factorial(i - n))
    acc = c[7] * fall(7)
    for i in range(6, n - 1, -1):
        acc = dt(dt(acc * tau) + dt(c[i] * fall(i)))
    return acc


def flat_map(cx, cy, tau, params, dtype):
    """flat output -> ([x, y, theta, xd, yd, thetad], [u1, u2]), every operation in `dtype`, the reference's formulas and order"""
    dt = np.dtype(dtype).type
    m, r, I, g = (dt(v) for v in params)
    cx, cy, tau = np.asarray(cx, dtype), np.asarray(cy, dtype), dt(tau)
    x, y = _horner(cx, tau, 0, dt), _horner(cy, tau, 0, dt)
    x1, y1 = _horner(cx, tau, 1, dt), _horner(cy, tau, 1, dt)
    x2, y2 = _horner(cx, tau, 2, dt), _horner(cy, tau, 2, dt)
    x3, y3 = _horner(cx, tau, 3, dt), _horner(cy, tau, 3, dt)
    x4, y4 = _horner(cx, tau, 4, dt), _horner(cy, tau, 4, dt)
    den = y2 + g
    den2, den3 = den * den, den * den * den
    q = dt(1) + (x2 / den) * (x2 / den)
    w = x3 / den - x2 * y3 / den2
    theta = -np.arctan2(x2, den)
    theta_dot = dt(-1) / q * w
    theta_ddot = dt(2) * x2 / den / (q * q) * (w * w) - dt(1) / q * (x4 / den - x3 * y3 / den2 - x3 * y3 / den2 - x2 * y4 / den2 + dt(2) * x2 * y3 / den3)
    s, c = np.sin(theta), np.cos(theta)
    if s != 0:
        u1 = (I / r * theta_ddot - m / s * x2) / dt(2)
        u2 = (-I / r * theta_ddot - m / s * x2) / dt(2)
    else:
        u1 = (I / r * theta_ddot + m / c * (y2 + g)) / dt(2)
        u2 = (-I / r * theta_ddot + m / c * (y2 + g)) / dt(2)
    out = np.array([x, y, theta, x1, y1, theta_dot], dtype), np.array([u1, u2], dtype)
    assert out[0].dtype == dtype and all(np.asarray(v).dtype == dtype for v in (x, theta, theta_ddot, u1))
    return out


def update(t, cumulated_t, coeff, end_point, params, dtype=np.float64):
    """the planner's update(t): segment = last i with t >= cumulated_t[i]; past the last waypoint a hover at end_point with local time 0"""
    idx = int(np.nonzero(t >= np.asarray(cumulated_t, np.float64))[0][-1])
    if idx == len(cumulated_t) - 1:
        cx, cy = np.zeros(8), np.zeros(8)
        cx[0], cy[0] = end_point
        tau = 0.0
    else:
        cx, cy = coeff[0, idx], coeff[1, idx]
        tau = float(t) - float(cumulated_t[idx])
    return flat_map(cx, cy, tau, params, dtype)


def reference_grid(plan, params, steps, t0=0.0, dt=0.05, dtype=np.float64):
    """x_ref (steps, 6), u_ref (steps, 2) at t_k = t0 + k dt"""
    out = [update(t0 + k * dt, plan["cumulated_t"], plan["coeff"], plan["waypoints"][-1], params, dtype) for k in range(steps)]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


# ---- the closed loop ------------------------------------------------------------------------------------------------------------------------
def wrap_angle(th, dt):
    pi, two_pi = dt(np.pi), dt(2 * np.pi)
    return dt(np.remainder(dt(th + pi), two_pi)) - pi


def xdot(x, u, params, dt):
    m, r, I, g = (dt(v) for v in params)
    s, c = np.sin(x[2]), np.cos(x[2])
    return np.array([x[3], x[4], x[5], dt(0) + (-s / m * u[0] + -s / m * u[1]), -g + (c / m * u[0] + c / m * u[1]),
                     dt(0) + (r / I * u[0] + -(r / I) * u[1])], dtype=dt)


def step(x, u, params, h, dt, rk4):
    if not rk4:
        xn = x + xdot(x, u, params, dt) * h
    else:
        k1 = xdot(x, u, params, dt)
        k2 = xdot(x + (h / dt(2)) * k1, u, params, dt)
        k3 = xdot(x + (h / dt(2)) * k2, u, params, dt)
        k4 = xdot(x + h * k3, u, params, dt)
        xn = x + (h / dt(6)) * (k1 + dt(2) * k2 + dt(2) * k3 + k4)
    xn = np.array(xn, dtype=dt)
    xn[2] = wrap_angle(xn[2], dt)
    return xn


def tracking_loop(plan, x0, steps, K, Q, R, umin, umax, params, t0=0.0, h=0.05, dtype=np.float64, rk4=False):
    """u_k = clip(u_ref(t_k) - K wrap(x_k - x_ref(t_k))), x_{k+1} = simulate(x_k, u_k) for ONE start state.
    -> dict traj (steps + 1, 6), u (steps, 2), cost (steps,), x_ref, u_ref"""
    dt = np.dtype(dtype).type
    K, Q, R, umin, umax = (np.asarray(a, dtype) for a in (K, Q, R, umin, umax))
    x = np.asarray(x0, dtype).copy()
    hd = dt(h)
    traj, us, cost, xrs, urs = [x.copy()], [], [], [], []
    for k in range(steps):
        xr, ur = update(t0 + k * h, plan["cumulated_t"], plan["coeff"], plan["waypoints"][-1], params, dtype)
        e = (x - xr).astype(dtype)
        e[2] = wrap_angle(e[2], dt)
        ke = np.zeros(2, dtype)
        for j in range(2):
            acc = dt(0)
            for i in range(6):
                acc = dt(acc + dt(K[j, i] * e[i]))
            ke[j] = acc
        u = np.clip(ur - ke, umin, umax).astype(dtype)
        du = u - ur
        cost.append(dt((dt(e @ (Q @ e)) + dt(du @ (R @ du))) * hd))
        x = step(x, u, params, hd, dt, rk4)
        assert x.dtype == dtype and u.dtype == dtype
        traj.append(x.copy()); us.append(u); xrs.append(xr); urs.append(ur)
    return dict(traj=np.array(traj), u=np.array(us), cost=np.array(cost, dtype), x_ref=np.array(xrs), u_ref=np.array(urs))
