"""Helpers for inspecting a trained value function (reference utils/debug_helper.py): local minima of V by (damped) Newton steps, the
locally equivalent linear map of a ReLU network, and two LQR sanity checks.  The two network helpers run batched on the device: V and dV/dx
come from the fused value-gradient kernel, d2V/dx2 and dy/de from hjbx_value_hessian_f32 (controllers that do not use the fused kernels, e.g.
float64 ones, go through the torch closed forms of ValueFunctionApproximator); the LQR checks are NumPy.  local_optimal_x also takes a
controller with the soft-PD network (hjbx_softpd_value_hessian_f32); the equivalent linear map is for the bias-free PD network only."""
from typing import Tuple

import numpy as np
import torch

from ..dynamics.dynamics_basic import _from_device, _to_device


def _restore(t: torch.Tensor, like, one: bool, kind: str):
    """-> `t` in the container, dtype and rank `like` came in"""
    if isinstance(like, torch.Tensor):
        t = t.to(like.dtype) if like.dtype.is_floating_point else t
    elif np.asarray(like).dtype in (np.float32, np.float64):
        t = t.to(torch.float32 if np.asarray(like).dtype == np.float32 else torch.float64)
    return _from_device(t, one, kind)


def _value_grad_hessian(nn_policy, x: torch.Tensor):
    vf = nn_policy.value_function_approximator       # either head: both modules have fused_value_grad / value_and_grad
    if nn_policy.fused_value_grad and x.dtype == torch.float32:
        V, g = vf.fused_value_grad(x)
    else:
        V, g = vf.value_and_grad(x)
    return V, g, nn_policy.value_hessian(x)


@torch.no_grad()
def local_optimal_x(x, nn_policy, max_iter=10, lr=1e-1, verbose=True, newton_method=True):
    """Iterate towards a local minimum of V near x (debug_helper.py:40-59).  x: (n,) or (B, n), tensor or array; all B starts advance at
    once on the device.  Per start and iteration: x <- x - lr H^-1 dV/dx where det H > 0 and `newton_method` is set, else x <- x - lr dV/dx
    (H = d2V/dx2).  verbose prints every iteration for a single start and a summary for a batch.  Returns x as it was given (type, shape)."""
    nn_policy.train_mode = False
    t, one, kind = _to_device(x, like_dtype=nn_policy.dtype)
    t = t.clone()
    n = t.shape[-1]
    eye = torch.eye(n, dtype=t.dtype, device=t.device)
    for i in range(int(max_iter)):
        V, g, H = _value_grad_hessian(nn_policy, t)
        if newton_method:
            newton = torch.linalg.det(H) > 0
            step = torch.linalg.solve(torch.where(newton[:, None, None], H, eye), g.unsqueeze(-1)).squeeze(-1)   # (identity: the gradient step)
        else:
            newton = torch.zeros(t.shape[0], dtype=torch.bool, device=t.device)
            step = g
        if verbose:
            if t.shape[0] == 1:
                u = nn_policy.get_control_efforts(t)
                print(f"iter:{i}, x: {t[0].cpu().numpy()}, value:{float(V[0]):.5f}, \n u:{u[0].cpu().numpy()} v_gradient:{g[0].cpu().numpy()} \n hess:{H[0].cpu().numpy()}")
            else:
                print(f"iter:{i}, starts:{t.shape[0]}, value mean:{float(V.mean()):.5f} max:{float(V.max()):.5f}, "
                      f"|v_gradient| max:{float(g.abs().max()):.3e}, newton steps:{int(newton.sum())}")
        t = t - lr * step
    return _restore(t, x, one, kind)


@torch.no_grad()
def get_equivalent_matrix_multiplication_for_fully_connected_nn(x, value_function_approximator) -> Tuple[np.ndarray, np.ndarray]:
    """(W, b) with y = W' e + b on the linear region of the ReLU network that contains x (debug_helper.py:7-38), y the output of the last layer
    and e = wrap(x - xf) the error coordinates.  x: (n,) or (B, n); W: (n, h3) or (B, n, h3), b: (h3,) or (B, h3).  W = dy/de from the Hessian
    kernel; the network has no biases, so y = W'(e - mean) exactly: b = -W' mean."""
    vf = value_function_approximator
    if not hasattr(vf, "weights"):
        raise ValueError("the equivalent linear map exists for the bias-free PD network, not for the soft-PD network (biases, scalar head)")
    if vf.activation != "relu":
        raise ValueError(f"the equivalent linear map exists for a ReLU network, this one uses {vf.activation!r}")
    dtype = vf.weights[0].dtype
    t, one, kind = _to_device(x, like_dtype=dtype)
    if dtype == torch.float32:
        W = vf.fused_value_hessian(t, want_jacobian=True)[1]
    else:
        W = vf.value_hessian(t, want_jacobian=True)[1]
    b = -(W.transpose(1, 2) @ vf.mean.to(W.dtype).unsqueeze(-1)).squeeze(-1)
    return _restore(W, x, one, kind), _restore(b, x, one, kind)


def check_controllability(A: np.ndarray, B: np.ndarray, verbose=False):
    """Kalman rank condition of the linear system x_dot = A x + B u: rank [B, AB, ..., A^(n-1) B] == n.
    verbose: -> (controllable, controllability matrix)."""
    A = np.asarray(A, np.float64)
    B = np.asarray(B, np.float64).reshape(A.shape[0], -1)
    blocks = [B]
    for _ in range(1, A.shape[0]):
        blocks.append(A @ blocks[-1])
    ctrb = np.hstack(blocks)
    controllable = bool(np.linalg.matrix_rank(ctrb) == A.shape[0])
    return (controllable, ctrb) if verbose else controllable


def check_hjb_condition_for_lqr(P: np.ndarray, A: np.ndarray, B: np.ndarray, Q: np.ndarray, R: np.ndarray, threshold=1e-5, verbose=False):
    """Does V = x'Px satisfy the differentiated HJB equation of the LQR problem?  True when one of the three residuals
        2 P'A - P'B R^-1 B'P + Q,    A'P + P'A - P'B R^-1 B'P + Q,    2 A'P - P'B R^-1 B'P + Q
    is below `threshold` in every entry (for a symmetric P the middle one is the algebraic Riccati equation).
    verbose: -> (satisfied, the three residuals)."""
    P, A, B, Q, R = (np.asarray(v, np.float64) for v in (P, A, B, Q, R))
    quad = P.T @ B @ np.linalg.solve(R, B.T @ P)
    residuals = (2.0 * P.T @ A - quad + Q, A.T @ P + P.T @ A - quad + Q, 2.0 * A.T @ P - quad + Q)
    satisfied = bool(any(np.max(np.abs(r)) < threshold for r in residuals))
    return (satisfied, *residuals) if verbose else satisfied
