"""The built-in linear systems at EVERY shape the library instantiates (TEST INFRASTRUCTURE, no GPU needed to import): besides the (2, 1)
of tests/offstock.py, (n, m) = (2, 2), (4, 1), (4, 2) and (6, 2) -- csrc/hjbx_host.hpp with_system.  With m = 1 a row-major B, a column-major
B and B with swapped columns are the same memory; the four configurations here have m = 2 wherever the library has it, and

  * every entry of A and B dyadic and non-zero, A != A', the |entries| of B pairwise distinct and its columns not proportional: a transposed
    read, a wrong row stride, a swapped column or a wrong offset into the parameter block changes B u;
  * dt = 1 / 32, asymmetric control and observation boxes, non-zero xf / uf, the dense Q, R, P and the mean / std of tests/offstock.py.

Importing this module adds the four names to the dictionaries of tests/offstock.py (no existing key changes), so its helpers -- stream_case,
step_sequence_case, rollout_case, box_states, offstock_task, make_offstock_dynamics, offstock_vhjb_config, product_controller -- and
the helpers of tests/test_gpu_offstock.py take them like any other system name.

tools/gen_golden_linear_shapes.py reads SHAPES / DT from here and writes tests/golden/linear_shapes.npz from the reference's code."""
import numpy as np

import offstock as OS

DT = OS.DT
NAMES = ["linear22", "linear41", "linear42", "linear62"]


def dense_A(n):
    """A_ij = ((3 i + 5 j) mod 7 - 2.5) / 4, minus 1 on the diagonal: odd multiples of 1 / 8 in [-1.625, 0.875], none zero, A != A'"""
    i, j = np.indices((n, n))
    return ((3 * i + 5 * j) % 7 - 2.5) / 4.0 - np.eye(n)


_B_ROWS = [[0.5, -0.25], [1.25, 0.75], [-0.375, 1.0], [0.625, -0.875], [0.125, 1.5], [-1.125, 0.3125]]
_B_COL = [[0.25], [-0.5], [1.0], [0.75]]
_XF = [0.25, -0.125, 0.5, -0.375, 0.0625, -0.25]
_OBS = ([-1.5, -3.0, -2.0, -2.5, -1.25, -2.0], [2.0, 2.5, 1.75, 3.0, 1.5, 2.5])
_LIMITS = {1: ([-3.0], [2.0]), 2: ([-2.5, -4.0], [3.0, 2.0])}
_UF = {1: [0.25], 2: [0.25, -0.5]}

SHAPES = {"linear22": (2, 2), "linear41": (4, 1), "linear42": (4, 2), "linear62": (6, 2)}
CONSTANTS = {name: dict(A=dense_A(n).tolist(), B=_B_COL if m == 1 else _B_ROWS[:n]) for name, (n, m) in SHAPES.items()}

for _name, (_n, _m) in SHAPES.items():
    OS.KIND[_name] = "linear"
    OS.CONSTANTS[_name] = CONSTANTS[_name]
    OS.LIMITS[_name] = _LIMITS[_m]
    OS.DIMS[_name] = (_n, _m)
    OS.XF[_name] = _XF[:_n]
    OS.UF[_name] = _UF[_m]
    OS.OBS[_name] = (_OBS[0][:_n], _OBS[1][:_n])


def matrices(name):
    """(A, B) float64"""
    c = CONSTANTS[name]
    return np.array(c["A"], np.float64), np.array(c["B"], np.float64)


def bang_task(name, target_r2=2.0 ** -6):
    """the shape's dense task with HJBX_LAW_BANGBANG: u_j = umax_j / umin_j by the sign of (f2' g)_j, unit running cost outside the target ball"""
    from q_learning_with_hjb_amd import _abi
    t = OS.offstock_task(name)
    t.law, t.target_r2 = _abi.LAW_BANGBANG, float(target_r2)
    return t


def handle_without_zoh(name):
    """a system handle of the shape created without Ad, Bd: the first half of the parameter block only"""
    from q_learning_with_hjb_amd import _abi
    n, m = SHAPES[name]
    h = OS.make_offstock_dynamics(name).system
    return _abi.SystemHandle(h.kind, n, m, h.dt, h.umin, h.umax, h.params[: n * n + n * m])


def oracle_system(name, A=None, B=None, Ad=None, Bd=None, umin=None, umax=None):
    """O.System of the shape with single matrices replaced (the sensitivity checks): the parameter block is A, B, Ad, Bd, each row-major"""
    from oracle import oracle as O
    from q_learning_with_hjb_amd import _abi
    n, m = SHAPES[name]
    A0, B0 = matrices(name)
    d = OS.make_offstock_dynamics(name)
    Ad0, Bd0 = d.A_d, d.B_d
    p = np.concatenate([np.asarray(v, np.float64).reshape(shape).ravel() for v, shape in
                        ((A0 if A is None else A, (n, n)), (B0 if B is None else B, (n, m)), (Ad0 if Ad is None else Ad, (n, n)),
                         (Bd0 if Bd is None else Bd, (n, m)))])
    lo, hi = OS.LIMITS[name]
    return O.System(_abi.SYS_LINEAR, n, m, DT, lo if umin is None else umin, hi if umax is None else umax, p)
