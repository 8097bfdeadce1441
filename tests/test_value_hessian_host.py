"""CPU-only tests of the value-network Hessian (hjbx_value_hessian_f32, csrc/hjbx_hessian.hip) and of utils/debug_helper.py:

  * the yardstick of the GPU tests, tests/hessref.py, against central finite differences of the gradient (NetRef.grad for ReLU, the reverse
    sweep of hessref for tanh / sin) in float64;
  * the argument checks of the entry point, one fault per call with made-up pointers in the style of test_mlp_entry_checks_host.py: every
    call must come back with its status and message BEFORE the device is touched;
  * the kernel metadata of the three compiled units (one per activation): no scratch, no spilled VGPR;
  * check_controllability and check_hjb_condition_for_lqr.
No compute call touches a GPU here."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, orc_system
from hessref import HessRef
from q_learning_with_hjb_amd import _abi
from q_learning_with_hjb_amd.utils.debug_helper import check_controllability, check_hjb_condition_for_lqr
from q_learning_with_hjb_amd.utils.utils import solve_continuous_are

OK, EINVAL, EUNSUPPORTED = _abi.OK, _abi.EINVAL, _abi.EUNSUPPORTED
CSRC = os.path.join(ROOT, "q_learning_with_hjb_amd", "csrc")
HIPCC = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=on"]
WHO = "hjbx_value_hessian_f32"


# ------------------------------------------------------------------------------------------------------------------------------------
# the yardstick
# ------------------------------------------------------------------------------------------------------------------------------------
def _lecun(rng, fan_in, fan_out):
    return (np.clip(rng.standard_normal((fan_in, fan_out)), -2, 2) / 0.87962566103423978 / np.sqrt(fan_in)).astype(np.float32).astype(np.float64)


def _wrap_second(e, dtype):
    """the second coordinate is an angle (the cart-pole's layout)"""
    e = np.array(e, dtype)
    if e.shape[1] > 1:
        e[:, 1] = (e[:, 1] + dtype(np.pi)) % dtype(2 * np.pi) - dtype(np.pi)
    return e


@pytest.mark.parametrize("activation", ["relu", "tanh", "sin"])
@pytest.mark.parametrize("n", [2, 4, 10])
def test_restated_hessian_equals_finite_differences_of_the_gradient(n, activation):
    """H of tests/hessref.py against central differences of dV/dx, float64, step 1e-6 (1 + |x_j|) along each coordinate, to 1e-6 of the
    sample's max |H|.  A central difference of a smooth gradient is off by h^2 |d3V| / 6 + 1e-16 |dV/dx| / h, about 1e-10 of max |H| here;
    the gradient of a ReLU network is piecewise linear, so away from the kinks (kink margin >= 1e-5, and no unit changes sign within any of
    the 2n steps) only the second term remains.  dy/de is checked the same way against central differences of y."""
    rng = np.random.default_rng(100 * n + len(activation))
    W = [_lecun(rng, n, 128), _lecun(rng, 128, 128), _lecun(rng, 128, 64)]
    mean, std, xf = 0.1 * rng.standard_normal(n), rng.uniform(0.5, 2.0, n), 0.3 * rng.standard_normal(n)
    ref = HessRef(W, mean, std, xf, 1e-3, _wrap_second, activation)
    x = xf[None, :] + rng.uniform(-1, 1, (200, n)) * 1.5
    if activation == "relu":
        def masks(q):
            fw = ref.net.forward(q)
            return np.concatenate([fw["a1"] > 0, fw["a2"] > 0], axis=1)
        same = ref.kink_margin(x) >= 1e-5
        for j in range(n):
            for sgn in (1.0, -1.0):
                xq = x.copy()
                xq[:, j] += sgn * 1e-6 * (1.0 + np.abs(x[:, j]))
                same &= (masks(xq) == masks(x)).all(1)
        x = x[same]
        assert x.shape[0] >= 150
        grad = lambda q: ref.net.grad(ref.net.forward(q))     # noqa: E731
    else:
        grad = ref.grad
    H, J = ref.hessian(x)
    assert H.shape == (x.shape[0], n, n) and J.shape == (x.shape[0], n, 64)
    Hfd, Jfd = np.empty_like(H), np.empty_like(J)
    for j in range(n):
        h = 1e-6 * (1.0 + np.abs(x[:, j]))
        xp, xm = x.copy(), x.copy()
        xp[:, j] += h
        xm[:, j] -= h
        Hfd[:, :, j] = (grad(xp) - grad(xm)) / (xp[:, j] - xm[:, j])[:, None]
        Jfd[:, j, :] = (ref.forward(xp)["y"] - ref.forward(xm)["y"]) / (xp[:, j] - xm[:, j])[:, None]
    for got, fd in ((H, Hfd), (J, Jfd)):
        scale = np.abs(got).reshape(x.shape[0], -1).max(1)
        err = np.abs(got - fd).reshape(x.shape[0], -1).max(1) / scale
        assert err.max() <= 1e-6, float(err.max())
    assert np.abs(H - H.transpose(0, 2, 1)).max() <= 1e-12 * np.abs(H).max()
    # the float32 evaluation of the same statements stays float32 and is close
    H32, J32 = ref.hessian(x, dtype=np.float32)
    assert H32.dtype == np.float32 and J32.dtype == np.float32
    if activation != "relu":
        assert np.abs(H32 - H).max() <= 1e-3 * np.abs(H).max()


# ------------------------------------------------------------------------------------------------------------------------------------
# argument checks
# ------------------------------------------------------------------------------------------------------------------------------------
PTR = 0x7F0000100000                    # made-up "device" addresses, 64 KiB apart
ADDR = {name: PTR + 0x10000 * k for k, name in enumerate(("x", "H", "dy", "W1", "W2", "W3"))}
USER_SRC = ("HJBX_DEV void wrap(T* x) const {}\n"
            "HJBX_DEV void affine(const T* x, T* f1, T* f2) const { for (int i = 0; i < 4; ++i) { f1[i] = x[i]; f2[i] = T(1); } }\n")
_systems = {}


def _system(name):
    if name not in _systems:
        if name == "user":
            _systems[name] = _abi.SystemHandle.from_source(_abi.USER_AFFINE, USER_SRC, 4, 1, 0.02, [-1], [1], [1.0])
        else:
            kind, n, m, npar = {"lin4": (_abi.SYS_LINEAR, 4, 1, 20), "lin6": (_abi.SYS_LINEAR, 6, 2, 48)}[name]
            _systems[name] = _abi.SystemHandle(kind, n, m, 0.02, -np.ones(m), np.ones(m), np.ones(npar))
    return _systems[name]


def _call(system="lin4", edit_mlp=None, **over):
    """One call with valid made-up arguments except what `edit_mlp` and `over` change -> (status, message)."""
    sys_h = _system(system)
    d = _abi.HjbxMlp()
    d.W1, d.W2, d.W3 = ADDR["W1"], ADDR["W2"], ADDR["W3"]
    d.h1, d.h2, d.h3, d.activation = 128, 128, 64, _abi.ACT_TANH
    for k in range(sys_h.n):
        d.std[k] = 1.0
    if edit_mlp:
        edit_mlp(d)
    a = dict(ADDR, sys=sys_h.ptr, mlp=_abi.ref(d), B=64)
    a.update(over)
    rc = _abi.lib().hjbx_value_hessian_f32(a["sys"], a["mlp"], a["x"], a["H"], a["dy"], a["B"], None)
    return rc, _abi.last_error()


def _set(**fields):
    return lambda d: [setattr(d, k, v) for k, v in fields.items()]


def _std_zero(d):
    d.std[3] = 0.0


ALIGN = "x must be aligned to its row vector width, H and dy_dx to 16 bytes"
FAULTS = [
    ("NULL system", dict(sys=None), EINVAL, "NULL system or mlp descriptor"),
    ("NULL network", dict(mlp=None), EINVAL, "NULL system or mlp descriptor"),
    ("negative B", dict(B=-1), EINVAL, "negative batch size"),
    ("NULL x", dict(x=None), EINVAL, "NULL x or weight pointer"),
    ("NULL W1", dict(edit_mlp=_set(W1=None)), EINVAL, "NULL x or weight pointer"),
    ("NULL W2", dict(edit_mlp=_set(W2=None)), EINVAL, "NULL x or weight pointer"),
    ("NULL W3", dict(edit_mlp=_set(W3=None)), EINVAL, "NULL x or weight pointer"),
    ("user-defined system", dict(system="user"), EUNSUPPORTED, "user-defined systems are not supported"),
    ("features", dict(edit_mlp=_set(h2=64)), EUNSUPPORTED, "features must be [128,128,64], got [128,64,64]"),
    ("activation 7", dict(edit_mlp=_set(activation=7)), EINVAL, "unknown activation 7"),
    ("x off 16 (n=4)", dict(x=ADDR["x"] + 8), EINVAL, ALIGN),
    ("x off 8 (n=6)", dict(system="lin6", x=ADDR["x"] + 4), EINVAL, ALIGN),
    ("H off 16", dict(H=ADDR["H"] + 8), EINVAL, ALIGN),
    ("H off 16 (n=6)", dict(system="lin6", H=ADDR["H"] + 8), EINVAL, ALIGN),
    ("dy_dx off 16", dict(dy=ADDR["dy"] + 4), EINVAL, ALIGN),
    ("H off 16, dy_dx NULL", dict(H=ADDR["H"] + 8, dy=None), EINVAL, ALIGN),
    ("std[3] = 0", dict(edit_mlp=_std_zero), EINVAL, "normalization_std[3] is zero"),
]


@pytest.mark.parametrize("kw, status, fragment", [pytest.param(kw, st, fr, id=name) for name, kw, st, fr in FAULTS])
def test_fault_is_rejected_before_the_device(kw, status, fragment):
    rc, msg = _call(**kw)
    assert rc == status, (rc, msg)
    assert msg.startswith(WHO + ": "), msg
    assert fragment in msg, msg


@pytest.mark.parametrize("kw", [dict(B=0), dict(H=None, dy=None), dict(B=0, x=None), dict(H=None, dy=None, system="user")],
                         ids=["B == 0", "both outputs NULL", "B == 0, NULL x", "both outputs NULL, user system"])
def test_nothing_to_compute_is_ok(kw):
    rc, msg = _call(**kw)
    assert rc == OK, msg


def test_symbol_and_header():
    hdr = open(os.path.join(ROOT, "include", "hjbx.h")).read()
    assert "hjbx_value_hessian_f32" in _abi.EXPORTED_SYMBOLS and hasattr(_abi.lib(), "hjbx_value_hessian_f32")
    assert re.search(r"^#define HJBX_HAS_VALUE_HESSIAN 1", hdr, flags=re.M) and re.search(r"^int hjbx_value_hessian_f32\(", hdr, flags=re.M)
    body = hdr[hdr.index("The Hessian of the PD value network"):hdr.index("int hjbx_value_hessian_f32(")]
    for cite in ("debug_helper.py:40-59", ":7-38", "debug_plots.py:145-172", "NOT bitwise symmetric"):
        assert cite in body, cite
    assert ("hjbx_hessian.hip", ("-DHJBX_HESS_ACT=1",), "hjbx_hessian_tanh.o") in _abi._UNITS


# ------------------------------------------------------------------------------------------------------------------------------------
# the compiled units
# ------------------------------------------------------------------------------------------------------------------------------------
def test_hessian_kernels_have_no_scratch_and_no_spilled_vgpr(tmp_path):
    """hjbx_hessian.hip, once per activation: seven instantiations each (the systems hjbx_value_grad_f32 dispatches), no scratch, no spilled
    VGPR; the kernel's name contains neither k_value_grad_mfma nor k_vhjb_rollout_mfma (other host tests count those) nor MlpHeadSoft (the
    same kernel with the other head is hjbx_softpd_hessian.hip's), and the inline-asm
    LDS reads of the chains pass the audits of tools/audit_asm_loads.py."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import audit_asm_loads
    outs, procs = [], []
    for act in (0, 1, 2):
        asm = tmp_path / f"hessian_act{act}.s"
        outs.append(asm)
        procs.append(subprocess.Popen(HIPCC + ["-S", "--cuda-device-only", f"-DHJBX_HESS_ACT={act}", "-o", str(asm), os.path.join(CSRC, "hjbx_hessian.hip")],
                                      stderr=subprocess.DEVNULL))
    for pr in procs:
        assert pr.wait() == 0
    meta = re.compile(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.sgpr_spill_count:\s+(\d+)\n"
                      r"(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)")
    for act, asm in enumerate(outs):
        text = asm.read_text()
        kernels = meta.findall(text)
        assert len(kernels) == 7 and all("k_value_hessian" in k[0] for k in kernels), [k[0] for k in kernels]
        assert not any("k_value_grad_mfma" in k[0] or "k_vhjb_rollout_mfma" in k[0] or "MlpHeadSoft" in k[0] for k in kernels)
        for name, private, _sgpr_spill, vgpr_spill in kernels:
            assert int(private) == 0 and int(vgpr_spill) == 0, f"{name}: {private} bytes of scratch, {vgpr_spill} spilled VGPRs"
        # relu: 7 of the 10 chains (no reverse sweep of the sample): 64 x 4 x 3 + 64 x 2 + 32 x 4 MFMAs at least, per instantiation
        assert text.count("v_mfma_f32_32x32x2_f32") >= 7 * (1024 if act == 0 else 1536)
        assert audit_asm_loads.audit(str(asm)) == 0
        assert audit_asm_loads.audit_mfma_asm_reads(str(asm)) == 0


# ------------------------------------------------------------------------------------------------------------------------------------
# the LQR checks of utils/debug_helper.py
# ------------------------------------------------------------------------------------------------------------------------------------
def test_check_controllability():
    A, B = np.array([[0.0, 1.0], [0.0, 0.0]]), np.array([[0.0], [1.0]])
    assert check_controllability(A, B) is True
    ok, ctrb = check_controllability(A, B, verbose=True)
    assert ok and np.array_equal(ctrb, np.array([[0.0, 1.0], [1.0, 0.0]]))
    # the second mode is neither driven nor coupled to the first
    A2, B2 = np.array([[-1.0, 0.0], [0.0, -2.0]]), np.array([[1.0], [0.0]])
    assert check_controllability(A2, B2) is False
    # two integrators in a chain driven at the wrong end
    assert check_controllability(A, np.array([[1.0], [0.0]])) is False


def _cartpole_linearisation():
    """(A, B) of the cart-pole at the upright by central differences of the CPU oracle's x_dot (float64)."""
    from oracle import oracle as O
    s = orc_system("cartpole")
    xf, uf, h = np.array([0.0, np.pi, 0.0, 0.0]), np.array([0.0]), 1e-6
    X, U = np.tile(xf, (10, 1)), np.tile(uf, (10, 1))
    for i in range(4):
        X[2 * i, i] += h
        X[2 * i + 1, i] -= h
    U[8, 0] += h
    U[9, 0] -= h
    J = (O.dynamics_step(s, X, U)[0::2] - O.dynamics_step(s, X, U)[1::2]) / (2 * h)
    return J[:4].T.copy(), J[4:].T.copy()


def test_check_hjb_condition_for_lqr():
    A, B = _cartpole_linearisation()
    Q, R = np.eye(4), np.eye(1)
    assert check_controllability(A, B)
    P = solve_continuous_are(A, B, Q, R)
    assert check_hjb_condition_for_lqr(P, A, B, Q, R) is True
    assert check_hjb_condition_for_lqr(1.1 * P, A, B, Q, R) is False
    ok, c1, c2, c3 = check_hjb_condition_for_lqr(P, A, B, Q, R, verbose=True)
    assert ok and np.abs(c2).max() < 1e-5 and c1.shape == c2.shape == c3.shape == (4, 4)
    # the middle residual is the Riccati equation; the outer two are not symmetric in A and fail for this P
    assert np.abs(c1).max() > 1e-3 and np.abs(c3).max() > 1e-3
