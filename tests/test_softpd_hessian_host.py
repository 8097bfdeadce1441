"""CPU-only tests of the soft-PD value network's Hessian (hjbx_softpd_value_hessian_f32, csrc/hjbx_softpd_hessian.hip):

  * the yardstick of the GPU tests, tests/softhessref.py, against central finite differences of its own gradient in float64;
  * SoftPDValueFunctionApproximator.value_hessian_error (the torch closed form) in float64 against the yardstick;
  * the argument checks of the entry point, one fault per call with made-up pointers in the style of test_value_hessian_host.py, and pairs of
    faults that pin the ORDER of the checks: every call must come back with its status and message BEFORE the device is touched;
  * the symbol, the header and the build units;
  * the kernel metadata of the two compiled units (tanh, sin): seven kernels each (the systems the value gradient dispatches), no scratch, no spilled
    VGPR, and the inline-asm audits of tools/audit_asm_loads.py.
No compute call touches a GPU here."""
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from conftest import ROOT
from softhessref import SoftHessRef
from q_learning_with_hjb_amd import _abi
from q_learning_with_hjb_amd.controller.vhjb import SoftPDValueFunctionApproximator

OK, EINVAL, EUNSUPPORTED = _abi.OK, _abi.EINVAL, _abi.EUNSUPPORTED
CSRC = os.path.join(ROOT, "q_learning_with_hjb_amd", "csrc")
HIPCC = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=on"]
WHO = "hjbx_softpd_value_hessian_f32"


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


def _network(rng, n):
    """lecun-normal kernels, NON-ZERO biases on every layer, mean != 0, std != 1"""
    params = [_lecun(rng, n, 128), rng.uniform(-0.5, 0.5, 128), _lecun(rng, 128, 128), rng.uniform(-0.5, 0.5, 128), _lecun(rng, 128, 64),
              rng.uniform(-0.5, 0.5, 64), _lecun(rng, 64, 1), rng.uniform(-0.5, 0.5, 1)]
    return params, 0.1 * rng.standard_normal(n), rng.uniform(0.5, 2.0, n), 0.3 * rng.standard_normal(n)


@pytest.mark.parametrize("activation", ["tanh", "sin"])
@pytest.mark.parametrize("n", [2, 4, 6, 10])
def test_restated_hessian_equals_finite_differences_of_the_gradient(n, activation):
    """H of tests/softhessref.py against central differences of its own dV/dx, float64, step 1e-6 (1 + |x_j|) along each coordinate, to 1e-6
    of the sample's max |H| -- the bound of test_value_hessian_host.py, derived the same way: a central difference of a smooth gradient is off
    by h^2 |d3V| / 6 + 1e-16 |dV/dx| / h, about 1e-10 of max |H| for these O(1) networks; 1e-6 leaves four decades for a sample whose max |H|
    is small next to its gradient, and is still six decades below any wrong term of the closed form."""
    rng = np.random.default_rng(100 * n + len(activation))
    params, mean, std, xf = _network(rng, n)
    ref = SoftHessRef(params, mean, std, xf, _wrap_second, activation)
    x = xf[None, :] + rng.uniform(-1, 1, (200, n)) * 1.5
    H = ref.hessian(x)
    assert H.shape == (200, n, n) and H.dtype == np.float64
    Hfd = np.empty_like(H)
    for j in range(n):
        h = 1e-6 * (1.0 + np.abs(x[:, j]))
        xp, xm = x.copy(), x.copy()
        xp[:, j] += h
        xm[:, j] -= h
        Hfd[:, :, j] = (ref.grad(xp) - ref.grad(xm)) / (xp[:, j] - xm[:, j])[:, None]
    scale = np.abs(H).reshape(200, -1).max(1)
    err = np.abs(H - Hfd).reshape(200, -1).max(1) / scale
    print(f"    n={n} {activation}: max |H - central difference| / sample max |H| = {err.max():.2e}")
    assert err.max() <= 1e-6, float(err.max())
    assert np.abs(H - H.transpose(0, 2, 1)).max() <= 1e-12 * np.abs(H).max()
    # the gradient itself: central differences of V
    g = ref.grad(x)
    gfd = np.empty_like(g)
    for j in range(n):
        h = 1e-6 * (1.0 + np.abs(x[:, j]))
        xp, xm = x.copy(), x.copy()
        xp[:, j] += h
        xm[:, j] -= h
        gfd[:, j] = (ref.value(xp) - ref.value(xm)) / (xp[:, j] - xm[:, j])
    assert (np.abs(g - gfd).max(1) / np.abs(g).max(1)).max() <= 1e-6
    # the float32 evaluation of the same statements stays float32 and is close
    H32 = ref.hessian(x, dtype=np.float32)
    assert H32.dtype == np.float32 and np.abs(H32 - H).max() <= 1e-3 * np.abs(H).max()


def test_restated_relu_hessian_is_zero():
    rng = np.random.default_rng(5)
    params, mean, std, xf = _network(rng, 4)
    ref = SoftHessRef(params, mean, std, xf, _wrap_second, "relu")
    assert not ref.hessian(xf[None, :] + rng.uniform(-1, 1, (50, 4))).any()


@pytest.mark.parametrize("activation", ["relu", "tanh", "sin"])
@pytest.mark.parametrize("n", [2, 4, 6, 10])
def test_module_closed_form_f64_equals_the_restatement(n, activation):
    """SoftPDValueFunctionApproximator.value_hessian_error in float64 on the CPU (constructed without a system, as test_softpd_host.py does)
    against the restatement: the same closed form in the same precision, to 1e-12 of the sample's max |H|."""
    rng = np.random.default_rng(7 * n + len(activation))
    params, mean, std, _ = _network(rng, n)
    vf = SoftPDValueFunctionApproximator(types.SimpleNamespace(state_dim=n), (128, 128, 64), mean, std, [0.0] * n, dtype=torch.float64,
                                         activation=activation)
    with torch.no_grad():
        for p, v in zip(vf.layers, params):
            p.copy_(torch.as_tensor(v, dtype=torch.float64).reshape(p.shape))
    ref = SoftHessRef(params, mean, std, np.zeros(n), lambda e, dtype: e, activation)
    e = rng.uniform(-1, 1, (100, n)) * 1.5
    H = vf.value_hessian_error(torch.as_tensor(e))
    assert H.dtype == torch.float64 and tuple(H.shape) == (100, n, n)
    want = ref.hessian(e)
    if activation == "relu":
        assert not H.numpy().any() and not want.any()
        return
    scale = np.abs(want).reshape(100, -1).max(1)
    assert (np.abs(H.numpy() - want).reshape(100, -1).max(1) / scale).max() <= 1e-12


# ------------------------------------------------------------------------------------------------------------------------------------
# argument checks
# ------------------------------------------------------------------------------------------------------------------------------------
PTR = 0x7F0000100000                    # made-up "device" addresses, 64 KiB apart
NAMES = ("x", "H", "W1", "b1", "W2", "b2", "W3", "b3", "w4", "b4")
ADDR = {name: PTR + 0x10000 * k for k, name in enumerate(NAMES)}
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
    d = _abi.HjbxSoftpdMlp()
    for name in NAMES[2:]:
        setattr(d, name, ADDR[name])
    d.h1, d.h2, d.h3, d.activation = 128, 128, 64, _abi.ACT_TANH
    for k in range(sys_h.n):
        d.std[k] = 1.0
    if edit_mlp:
        edit_mlp(d)
    a = dict(x=ADDR["x"], H=ADDR["H"], sys=sys_h.ptr, mlp=_abi.ref(d), B=64)
    a.update(over)
    rc = _abi.lib().hjbx_softpd_value_hessian_f32(a["sys"], a["mlp"], a["x"], a["H"], a["B"], None)
    return rc, _abi.last_error()


def _set(**fields):
    return lambda d: [setattr(d, k, v) for k, v in fields.items()]


def _std_zero(d):
    d.std[3] = 0.0


def _both(*edits):
    return lambda d: [e(d) for e in edits]


NULLP = "NULL x, weight or bias pointer"
USER = "user-defined systems are not supported"
ALIGN = "x must be aligned to its row vector width, H to 16 bytes"
FEATURES = "features must be [128,128,64], got [128,64,64]"
FAULTS = [
    ("NULL system", dict(sys=None), EINVAL, "NULL system or mlp descriptor"),
    ("NULL network", dict(mlp=None), EINVAL, "NULL system or mlp descriptor"),
    ("negative B", dict(B=-1), EINVAL, "negative batch size"),
    ("NULL x", dict(x=None), EINVAL, NULLP),
] + [(f"NULL {name}", dict(edit_mlp=_set(**{name: None})), EINVAL, NULLP) for name in NAMES[2:]] + [
    ("user-defined system", dict(system="user"), EUNSUPPORTED, USER),
    ("features", dict(edit_mlp=_set(h2=64)), EUNSUPPORTED, FEATURES),
    ("activation 7", dict(edit_mlp=_set(activation=7)), EINVAL, "unknown activation 7"),
    ("x off 16 (n=4)", dict(x=ADDR["x"] + 8), EINVAL, ALIGN),
    ("x off 8 (n=6)", dict(system="lin6", x=ADDR["x"] + 4), EINVAL, ALIGN),
    ("H off 16", dict(H=ADDR["H"] + 8), EINVAL, ALIGN),
    ("H off 16 (n=6)", dict(system="lin6", H=ADDR["H"] + 4), EINVAL, ALIGN),
    ("std[3] = 0", dict(edit_mlp=_std_zero), EINVAL, "normalization_std[3] is zero"),
    # two faults at once: the earlier check answers
    ("negative B before NULL x", dict(B=-1, x=None), EINVAL, "negative batch size"),
    ("NULL b3 before the user system", dict(system="user", edit_mlp=_set(b3=None)), EINVAL, NULLP),
    ("user system before the features", dict(system="user", edit_mlp=_set(h2=64)), EUNSUPPORTED, USER),
    ("features before the activation", dict(edit_mlp=_set(h2=64, activation=7)), EUNSUPPORTED, FEATURES),
    ("activation before the alignment", dict(edit_mlp=_set(activation=7), x=ADDR["x"] + 8), EINVAL, "unknown activation 7"),
    ("alignment before std", dict(edit_mlp=_std_zero, H=ADDR["H"] + 8), EINVAL, ALIGN),
    ("relu is checked like the others", dict(edit_mlp=_both(_set(activation=_abi.ACT_RELU), _std_zero)), EINVAL, "normalization_std[3] is zero"),
]


@pytest.mark.parametrize("kw, status, fragment", [pytest.param(kw, st, fr, id=name) for name, kw, st, fr in FAULTS])
def test_fault_is_rejected_before_the_device(kw, status, fragment):
    rc, msg = _call(**kw)
    assert rc == status, (rc, msg)
    assert msg.startswith(WHO + ": "), msg
    assert fragment in msg, msg


@pytest.mark.parametrize("kw", [dict(B=0), dict(H=None), dict(B=0, x=None), dict(H=None, system="user"), dict(H=None, edit_mlp=_set(W2=None))],
                         ids=["B == 0", "H NULL", "B == 0, NULL x", "H NULL, user system", "H NULL, NULL W2"])
def test_nothing_to_compute_is_ok(kw):
    rc, msg = _call(**kw)
    assert rc == OK, msg


def test_symbol_header_and_units():
    hdr = open(os.path.join(ROOT, "include", "hjbx.h")).read()
    assert WHO in _abi.EXPORTED_SYMBOLS and hasattr(_abi.lib(), WHO)
    assert re.search(r"^#define HJBX_HAS_SOFTPD_VALUE_HESSIAN 1", hdr, flags=re.M) and re.search(rf"^int {WHO}\(", hdr, flags=re.M)
    assert int(re.search(r"#define HJBX_VERSION (\d+)", hdr).group(1)) == 112 == _abi.lib().hjbx_version()
    typed = hdr[hdr.index("#define HJBX_DECLARE"):hdr.index("HJBX_DECLARE(float, f32)")]
    assert "softpd" not in typed
    body = hdr[hdr.index("The Hessian of the soft-PD value network"):hdr.index(f"int {WHO}(")]
    for cite in ("debug_helper.py:40-59", "symmetric up to rounding, not bitwise", "fills H with zeros", "d3. = w4 . act''(a3) . a3."):
        assert cite in body, cite
    assert ("hjbx_softpd_hessian.hip", ("-DHJBX_SOFTPD_HESS_ACT=1",), "hjbx_softpd_hessian_tanh.o") in _abi._UNITS
    assert ("hjbx_softpd_hessian.hip", ("-DHJBX_SOFTPD_HESS_ACT=2",), "hjbx_softpd_hessian_sin.o") in _abi._UNITS
    assert "hjbx_hessian_kernels.hpp" in _abi._HEADERS


# ------------------------------------------------------------------------------------------------------------------------------------
# the compiled units
# ------------------------------------------------------------------------------------------------------------------------------------
def test_softpd_hessian_kernels_have_no_scratch_and_no_spilled_vgpr(tmp_path):
    """hjbx_softpd_hessian.hip, once per smooth activation: seven instantiations of k_value_hessian with the soft-PD head each (the systems
    hjbx_softpd_value_grad_f32 dispatches), no scratch, no spilled VGPR -- this is what keeps a (system, activation) pair that does not fit
    the register file out of the library -- and the inline-asm LDS reads of the chains pass the audits of tools/audit_asm_loads.py."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import audit_asm_loads
    outs, procs = {}, []
    for act in (_abi.ACT_TANH, _abi.ACT_SIN):
        outs[act] = tmp_path / f"softpd_hessian_act{act}.s"
        procs.append(subprocess.Popen(HIPCC + ["-S", "--cuda-device-only", f"-DHJBX_SOFTPD_HESS_ACT={act}", "-o", str(outs[act]),
                                               os.path.join(CSRC, "hjbx_softpd_hessian.hip")], stderr=subprocess.DEVNULL))
    for pr in procs:
        assert pr.wait() == 0
    meta = re.compile(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.sgpr_spill_count:\s+(\d+)\n"
                      r"(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)")
    for act, asm in outs.items():
        kernels = meta.findall(asm.read_text())
        assert len(kernels) == 7 and all("k_value_hessian" in k[0] and "MlpHeadSoft" in k[0] for k in kernels), [k[0] for k in kernels]
        for name, private, _sgpr_spill, vgprs, vgpr_spill in kernels:
            print(f"    act {act} {name[:64]}: {vgprs} VGPRs")
            assert int(private) == 0 and int(vgpr_spill) == 0, f"{name}: {private} bytes of scratch, {vgpr_spill} spilled VGPRs"
            assert int(vgprs) <= 512
        assert audit_asm_loads.audit(str(asm)) == 0
        assert audit_asm_loads.audit_mfma_asm_reads(str(asm)) == 0
