"""GPU tests of the value-network Hessian for user-defined systems: hjbx_value_hessian_f32 / hjbx_softpd_value_hessian_f32 on a handle that
asked for the matrix-core kernels run k_value_hessian compiled at first use for the user's struct (csrc/hjbx_user_hessian_kernels.hpp).

  * bit for bit: the user planar quadrotor (its wrap is the built-in one) against the built-in Quadrotors2D kernel -- same template, same flags;
  * parity at n = 8, a state dimension no built-in system has (C = 32 / n = 4 samples fill all 32 columns of a tile), and at n = 10, against
    tests/hessref.py / tests/softhessref.py with a NumPy restatement of wrap_angle.  Yardstick as in test_gpu_value_hessian.py: error per sample
    relative to that sample's own max |H_ref|; max and p99 within 2 x the CPU float32 evaluation of the same statements (floor 2^-24); states
    within 1e-5 of the wrap seam and, for ReLU, with kink margin < 1e-5 are left out, at most 2 % (asserted);
  * tile edges at n = 8 with sentinel rows behind each output; soft-PD ReLU (zeros, nothing compiled);
  * the controller: VHJBController.value_hessian takes the kernel for such a system, local_optimal_x works on it, a user system without
    matrix_cores keeps the torch closed form, and a unit the library refuses (scratch) falls back to it and is remembered.
The network is given by descriptors built from this file's own weights (lecun normal, mean != 0, std != 1); all of them float32 numbers."""
import json
import os
import time
import types

import numpy as np
import pytest
import torch

from conftest import ROOT, make_vhjb_config
from hessref import HessRef
from softhessref import SoftHessRef
from q_learning_with_hjb_amd import _abi, _ops
from q_learning_with_hjb_amd.configs import defaults as D
from q_learning_with_hjb_amd.controller.vhjb import VHJBController
from q_learning_with_hjb_amd.dynamics.quadrotors import Quadrotors2D
from q_learning_with_hjb_amd.utils.debug_helper import local_optimal_x
from test_gpu_user_system import CFG, UserCartpole, UserQuad2D
from test_user_fused_host import FusedCartpole, FusedQuad2D, Manip10
from test_user_hessian_host import SCRATCH_SRC, n8_handle

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
B_FULL = 1000                                   # not a multiple of any C = 32 // n and not of 32
KINK = 1e-5
SENTINEL = 12345.678
ACT = {"relu": _abi.ACT_RELU, "tanh": _abi.ACT_TANH, "sin": _abi.ACT_SIN}

_systems, _nets, _refs, _report = {}, {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    if not _report:
        return
    path = os.path.join(ROOT, "profiles", "user_value_hessian.json")
    try:
        old = {}
        if os.path.exists(path):
            with open(path) as f:
                old = json.load(f)
        old.setdefault("parity", {}).update(_report)
        with open(path, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)
    except OSError:
        pass


def system(name):
    """one handle per system for the whole file (a Hessian unit is compiled once per handle): -> (handle, angle coordinates)"""
    if name not in _systems:
        if name == "n8":
            _systems[name] = (None, n8_handle(), [1, 2])
        elif name == "quad2d":
            d = FusedQuad2D(D.quadrotors2d_dynamics_config())
            _systems[name] = (d, d.system, [2])
        elif name == "quad2d_builtin":
            d = Quadrotors2D(D.quadrotors2d_dynamics_config())
            _systems[name] = (d, d.system, [2])
        elif name == "manip10":
            d = Manip10(D.near_hover_dynamics_config())
            _systems[name] = (d, d.system, [1, 2])
    return _systems[name][1:]


def wrap_np(angle_idx):
    """wrap_angle of csrc/hjbx_systems.hpp on the listed coordinates, in `dtype`: np.remainder(th + pi, 2 pi) - pi"""
    def wrap(e, dtype):
        e = np.array(e, dtype)
        for k in angle_idx:
            e[:, k] = (e[:, k] + dtype(np.pi)) % dtype(2 * np.pi) - dtype(np.pi)
        return e
    return wrap


def _lecun(rng, fan_in, fan_out):
    return (np.clip(rng.standard_normal((fan_in, fan_out)), -2, 2) / 0.87962566103423978 / np.sqrt(fan_in)).astype(np.float32)


def net(n, angle_idx):
    """The test's own network and states for dimension n: weights of both heads (the soft-PD head shares W1..W3), normalisation, target, eps,
    B_FULL states around the target with the angles crossing the seam.  Made once, shared, never modified."""
    key = (n, tuple(angle_idx))
    if key not in _nets:
        rng = np.random.default_rng(1000 + n)
        W = [_lecun(rng, n, 128), _lecun(rng, 128, 128), _lecun(rng, 128, 64)]
        bias = [rng.uniform(-0.5, 0.5, 128).astype(np.float32), rng.uniform(-0.5, 0.5, 128).astype(np.float32),
                rng.uniform(-0.5, 0.5, 64).astype(np.float32)]
        w4, b4 = _lecun(rng, 64, 1), np.array([0.3], np.float32)
        mean = np.array([((k % 3) - 1) / 16.0 + 1.0 / 32.0 for k in range(n)])
        std = np.array([(0.75, 1.5, 1.25, 2.0, 0.5)[k % 5] for k in range(n)])
        xf = (0.3 * rng.standard_normal(n)).astype(np.float32).astype(np.float64)
        eps = float(np.float32(0.01))
        box = np.full(n, 3.0)
        box[angle_idx] = 1.25 * np.pi
        x32 = (xf + rng.uniform(-1, 1, (B_FULL, n)) * box).astype(np.float32)
        xr = x32.astype(np.float64)
        seam = np.ones(B_FULL, bool)
        for k in angle_idx:
            seam &= np.abs(np.abs(xr[:, k] - xf[k]) - np.pi) > 1e-5
        _nets[key] = types.SimpleNamespace(n=n, angle_idx=angle_idx, W=W, bias=bias, w4=w4, b4=b4, mean=mean, std=std, xf=xf, eps=eps, x32=x32, xr=xr,
                                           seam=seam, x=None)
    return _nets[key]


def on_device(c):
    """the device copies of the network and the states (the references above need none)"""
    if c.x is None:
        dev = lambda a: torch.as_tensor(a, device="cuda").contiguous()     # noqa: E731
        c.tW, c.tb, c.tw4, c.tb4, c.x = [dev(w) for w in c.W], [dev(b) for b in c.bias], dev(c.w4), dev(c.b4), dev(c.x32)
    return c


def descriptor(c, head, activation):
    on_device(c)
    d = _abi.HjbxSoftpdMlp() if head == "soft" else _abi.HjbxMlp()
    d.W1, d.W2, d.W3 = (t.data_ptr() for t in c.tW)
    if head == "soft":
        d.b1, d.b2, d.b3 = (t.data_ptr() for t in c.tb)
        d.w4, d.b4 = c.tw4.data_ptr(), c.tb4.data_ptr()
    else:
        d.eps_scalar = c.eps
    d.h1, d.h2, d.h3, d.activation = 128, 128, 64, ACT[activation]
    _abi._fill(d.mean, c.mean)
    _abi._fill(d.std, c.std)
    _abi._fill(d.xf, c.xf)
    return d


def reference(c, head, activation):
    """float64 and CPU-float32 closed forms and the kept states for (head, activation): computed once, shared, never modified"""
    key = (c.n, tuple(c.angle_idx), head, activation)
    if key not in _refs:
        wrap = wrap_np(c.angle_idx)
        W64 = [w.astype(np.float64) for w in c.W]
        keep = c.seam.copy()
        if head == "soft":
            ref = SoftHessRef([W64[0], c.bias[0], W64[1], c.bias[1], W64[2], c.bias[2], c.w4, c.b4], c.mean, c.std, c.xf, wrap, activation)
            H64, H32, J64, J32 = ref.hessian(c.xr), ref.hessian(c.xr, dtype=np.float32), None, None
        else:
            ref = HessRef(W64, c.mean, c.std, c.xf, c.eps, wrap, activation)
            if activation == "relu":
                keep &= ref.kink_margin(c.xr) >= KINK
            (H64, J64), (H32, J32) = ref.hessian(c.xr), ref.hessian(c.xr, dtype=np.float32)
        assert keep.mean() >= 0.98, f"n={c.n} {head} {activation}: {1 - keep.mean():.2%} of the states left out"
        _refs[key] = types.SimpleNamespace(ref=ref, keep=keep, H64=H64, H32=H32, J64=J64, J32=J32)
    return _refs[key]


def _rel_err(got, want):
    """|got - want| / (the sample's max |want|), per element"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = np.abs(want).reshape(want.shape[0], -1).max(1)
    return np.abs(got - want) / scale.reshape((-1,) + (1,) * (want.ndim - 1))


def _stats(err):
    return dict(max=float(err.max()), p99=float(np.quantile(err, 0.99)))


def _run(handle, c, head, activation, x=None):
    x = on_device(c).x if x is None else x
    if head == "soft":
        return _ops.softpd_value_hessian(handle, descriptor(c, head, activation), x), None
    return _ops.value_hessian(handle, descriptor(c, head, activation), x, True, True)


def _parity(tag, handle, c, head, activation):
    r = reference(c, head, activation)
    H, J = _run(handle, c, head, activation)
    torch.cuda.synchronize()
    assert H.shape == (B_FULL, c.n, c.n) and H.dtype == torch.float32 and (J is None or J.shape == (B_FULL, c.n, 64))
    H = H.cpu().numpy()
    outs = [("H", H, r.H32, r.H64)] + ([("dy_dx", J.cpu().numpy(), r.J32, r.J64)] if J is not None else [])
    line = {}
    for label, got, cpu, want in outs:
        assert np.isfinite(got).all()
        sg, sc = _stats(_rel_err(got, want)[r.keep]), _stats(_rel_err(cpu, want)[r.keep])
        line[label] = dict(kernel=sg, cpu_f32=sc, ratio_max=sg["max"] / max(sc["max"], U), ratio_p99=sg["p99"] / max(sc["p99"], U))
        print(f"    {tag} {head} {activation} {label}: err / sample scale  kernel max {sg['max']:.2e} p99 {sg['p99']:.2e} | CPU float32 max {sc['max']:.2e} "
              f"p99 {sc['p99']:.2e} | kernel / CPU: max {line[label]['ratio_max']:.2f} p99 {line[label]['ratio_p99']:.2f}")
    line["left_out"] = float(1 - r.keep.mean())
    _report[f"{tag}-{head}-{activation}"] = line
    for label in line:
        if label == "left_out":
            continue
        assert line[label]["kernel"]["max"] <= 2.0 * max(line[label]["cpu_f32"]["max"], U), (label, line[label])
        assert line[label]["kernel"]["p99"] <= 2.0 * max(line[label]["cpu_f32"]["p99"], U), (label, line[label])
    # symmetric up to rounding: twice the parity bound of the two elements
    asym = _rel_err(H, H.transpose(0, 2, 1))[r.keep].max()
    assert asym <= 4.0 * max(line["H"]["cpu_f32"]["max"], U), asym


# ------------------------------------------------------------------------------------------------------------------------------------
# bit for bit against the built-in kernel
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head, activation", [("pd", "relu"), ("pd", "tanh"), ("pd", "sin"), ("soft", "tanh")])
def test_user_quadrotor_is_the_builtin_kernel_bit_for_bit(head, activation):
    """The user planar quadrotor against Quadrotors2D on the same inputs: H and dy_dx (PD head), H (soft-PD tanh).  The kernel template, the
    wrap and the flags are the same, as for the value gradient in test_gpu_user_fused.py."""
    (hu, idx), (hb, _) = system("quad2d"), system("quad2d_builtin")
    assert hu.kind == _abi.SYS_USER and hu.matrix_cores and hb.kind == _abi.SYS_QUAD2D
    c = net(6, idx)
    Hu, Ju = _run(hu, c, head, activation)
    Hb, Jb = _run(hb, c, head, activation)
    assert torch.isfinite(Hb).all() and float(Hb.abs().max()) > 0
    assert torch.equal(Hu, Hb), f"H differs in {int((Hu != Hb).sum())} of {Hu.numel()} elements"
    if head == "pd":
        assert torch.equal(Ju, Jb), f"dy_dx differs in {int((Ju != Jb).sum())} of {Ju.numel()} elements"


# ------------------------------------------------------------------------------------------------------------------------------------
# parity where no built-in kernel exists
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head, activation", [("pd", "relu"), ("pd", "tanh"), ("pd", "sin"), ("soft", "sin")])
def test_parity_at_n8(head, activation):
    h, idx = system("n8")
    _parity("n8", h, net(8, idx), head, activation)


def test_parity_at_n10():
    h, idx = system("manip10")
    _parity("manip10", h, net(10, idx), "pd", "sin")


# ------------------------------------------------------------------------------------------------------------------------------------
# tile edges at n = 8: C = 4 samples per tile, no idle column
# ------------------------------------------------------------------------------------------------------------------------------------
def _raw_call(h, c, activation, x, B, want_h=True, want_j=True):
    """the PD entry point on buffers with 64 extra rows of a sentinel -> (H buffer, dy_dx buffer)"""
    Hb = torch.full((B + 64, c.n, c.n), SENTINEL, dtype=torch.float32, device="cuda")
    Jb = torch.full((B + 64, c.n, 64), SENTINEL, dtype=torch.float32, device="cuda")
    _abi.check(_abi.lib().hjbx_value_hessian_f32(h.ptr, _abi.ref(descriptor(c, "pd", activation)), x.data_ptr(), Hb.data_ptr() if want_h else None,
                                                 Jb.data_ptr() if want_j else None, B, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return Hb, Jb


@pytest.mark.parametrize("activation", ["relu", "tanh"])
def test_tile_edges_and_bounds_at_n8(activation):
    """Batches around the tile (4 samples) and the 32-sample boundaries: rows below B within the parity bound (2 x the CPU float32 build's max
    over the full batch), every sentinel row behind them bit-unchanged, either output alone bit-identical to the joint call, two launches
    bit-equal."""
    h, idx = system("n8")
    c = on_device(net(8, idx))
    r = reference(c, "pd", activation)
    sentinel = torch.tensor(SENTINEL, dtype=torch.float32).view(torch.int32).item()
    bound_h = 2.0 * max(_rel_err(r.H32, r.H64)[r.keep].max(), U)
    bound_j = 2.0 * max(_rel_err(r.J32, r.J64)[r.keep].max(), U)
    for B in (1, 3, 4, 5, 32, 33):
        x = c.x[:B].contiguous()
        Hb, Jb = _raw_call(h, c, activation, x, B)
        for buf in (Hb, Jb):
            assert bool((buf[B:].view(torch.int32) == sentinel).all()), f"B={B}: a row beyond the batch was written"
        keep = r.keep[:B]
        assert _rel_err(Hb[:B].cpu().numpy(), r.H64[:B])[keep].max(initial=0.0) <= bound_h, B
        assert _rel_err(Jb[:B].cpu().numpy(), r.J64[:B])[keep].max(initial=0.0) <= bound_j, B
        assert not bool((Hb[:B].view(torch.int32) == sentinel).any()) and not bool((Jb[:B].view(torch.int32) == sentinel).any())
        H1, J1 = _raw_call(h, c, activation, x, B, want_j=False)
        assert torch.equal(H1, Hb) and bool((J1.view(torch.int32) == sentinel).all())
        H2, J2 = _raw_call(h, c, activation, x, B, want_h=False)
        assert torch.equal(J2, Jb) and bool((H2.view(torch.int32) == sentinel).all())
        H3, J3 = _raw_call(h, c, activation, x, B)
        assert torch.equal(H3, Hb) and torch.equal(J3, Jb)


def test_softpd_relu_on_an_enabled_user_handle_is_zero_and_compiles_nothing():
    h = n8_handle()                      # a handle of its own: no Hessian unit has been compiled for it
    c = on_device(net(8, [1, 2]))
    _ops.softpd_value_hessian(system("n8")[0], descriptor(c, "soft", "relu"), c.x[:8].contiguous())     # (the memset path is warm)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    H = _ops.softpd_value_hessian(h, descriptor(c, "soft", "relu"), c.x)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert H.shape == (B_FULL, 8, 8) and not bool(H.view(torch.int32).any())
    assert dt < 0.5, f"{dt:.2f} s: a unit was compiled"


# ------------------------------------------------------------------------------------------------------------------------------------
# the controller and local_optimal_x
# ------------------------------------------------------------------------------------------------------------------------------------
def test_controller_takes_the_kernel_and_local_optimal_x_finds_the_target():
    """FusedCartpole with load_quadratic(P): the controller's value_hessian is the kernel's, bit for bit, and equals 2P + 2 eps I within the
    bound of test_quadratic_network_known_answer, |err|_ij <= (2n + 8) 2^-24 (2 (|L| |L|')_ij + 2 eps), P = L L'.  One full Newton step of
    local_optimal_x from 256 starts lands on xf within the backward-error bound of an n x n float32 solve per sample,
    64 x 2^-24 x cond_2(H) x |e0|_inf (test_local_optimal_x_on_a_quadratic_value_function); the starts are taken on xf's side of the wrap
    seam (beyond it the minimum of V in x is xf + 2 pi)."""
    d = FusedCartpole(D.cartpole_dynamics_config(**CFG))
    xf32 = [float(np.float32(v)) for v in make_vhjb_config("cartpole").xf]
    ctl = VHJBController(d, make_vhjb_config("cartpole", xf=xf32), dtype=torch.float32, activation="relu")
    vf = ctl.value_function_approximator
    vf.load_quadratic(ctl.P)
    assert d.system.kind == _abi.SYS_USER and d.system.matrix_cores and ctl.fused_value_grad and not ctl._user_hessian_refused
    n, eps = 4, vf.epsilon_scalar
    xf = np.asarray(ctl.xf, np.float64)
    rng = np.random.default_rng(11)
    box = np.asarray(ctl.obs_max, np.float64).clip(max=3.0)
    box[1] = 1.25 * np.pi
    x = torch.as_tensor((xf + rng.uniform(-1, 1, (B_FULL, n)) * box).astype(np.float32), device="cuda").contiguous()
    xr = x.cpu().numpy().astype(np.float64)
    W = [w.detach().cpu().numpy().astype(np.float64) for w in vf.weights]
    ref = HessRef(W, vf._np["mean"], vf._np["std"], vf._np["xf"], eps, wrap_np([1]), "relu")
    keep = np.abs(np.abs(xr[:, 1] - xf[1]) - np.pi) > 1e-5
    c1, c2 = ref.net.kink_candidates(ref.net.forward(xr), KINK)      # (units behind all-zero columns are exactly 0: not candidates)
    keep &= ~(c1.any(1) | c2.any(1))
    assert keep.mean() >= 0.98
    Hk = vf.fused_value_hessian(x)
    Hc = ctl.value_hessian(x)
    assert torch.equal(Hc, Hk) and not ctl._user_hessian_refused
    P = np.asarray(ctl.P, np.float64)
    L = np.linalg.cholesky(P)
    bound = (2 * n + 8) * U * (2.0 * np.abs(L) @ np.abs(L).T + 2.0 * eps)
    err = np.abs(Hk.cpu().numpy().astype(np.float64)[keep] - (2.0 * P + 2.0 * eps * np.eye(n))[None])
    print(f"    user cart-pole: max err / bound {float((err / bound[None]).max()):.3f} over {int(keep.sum())} states")
    assert (err <= bound[None]).all(), float((err / bound[None]).max())
    # local_optimal_x
    first = np.flatnonzero(keep & (np.abs(xr[:, 1] - xf[1]) < np.pi - 0.1))[:256]
    assert first.size == 256
    x0, x0r = x[torch.as_tensor(first, device="cuda")].contiguous(), xr[first]
    H0, _ = ref.hessian(x0r)
    tol = 64 * U * np.linalg.cond(H0, 2) * np.abs(x0r - xf[None]).max(1)
    x1 = local_optimal_x(x0, ctl, max_iter=1, lr=1.0, verbose=False, newton_method=True)
    assert isinstance(x1, torch.Tensor) and x1.is_cuda and x1.shape == x0.shape and x1.dtype == torch.float32
    off = np.abs(x1.cpu().numpy().astype(np.float64) - xf[None]).max(1)
    print(f"    local_optimal_x: max |x1 - xf| / tol {float((off / tol).max()):.3f}")
    assert (off <= tol).all(), float((off / tol).max())


def test_user_system_without_matrix_cores_keeps_the_closed_form():
    d = UserCartpole(D.cartpole_dynamics_config(**CFG))
    ctl = VHJBController(d, make_vhjb_config("cartpole"), dtype=torch.float32, activation="tanh")
    assert not d.system.matrix_cores and not ctl.fused_value_grad
    vf = ctl.value_function_approximator
    x = torch.as_tensor(np.asarray(ctl.xf, np.float64) + np.random.default_rng(3).uniform(-1, 1, (64, 4)), dtype=torch.float32, device="cuda").contiguous()
    assert torch.equal(ctl.value_hessian(x), vf.value_hessian(x))
    with pytest.raises(NotImplementedError, match="user-defined systems are not supported"):
        _ops.value_hessian(d.system, vf.descriptor(), x)


class ScratchQuad2D(UserQuad2D):
    """the planar quadrotor whose wrap needs private memory in the Hessian unit (test_user_hessian_host.py): that unit is refused"""

    def device_source(self):
        return dict(super().device_source(), source=SCRATCH_SRC, matrix_cores=True)


@pytest.mark.parametrize("structure", ["pd", "soft_pd"])
def test_controller_falls_back_and_remembers_when_the_unit_is_refused(structure):
    """Nothing of the refused kernel is launched: the library reports the scratch refusal, the controller returns the torch closed form --
    what it returned for this system before the kernel existed -- and does not ask again; fused_value_hessian itself raises."""
    if "scratch" not in _systems:
        _systems["scratch"] = ScratchQuad2D(D.quadrotors2d_dynamics_config())
    d = _systems["scratch"]
    ctl = VHJBController(d, make_vhjb_config("quad2d"), dtype=torch.float32, activation="tanh", value_structure=structure)
    assert d.system.matrix_cores and ctl.fused_value_grad
    vf = ctl.value_function_approximator
    x = torch.as_tensor(np.asarray(ctl.xf, np.float64) + np.random.default_rng(5).uniform(-1, 1, (64, 6)), dtype=torch.float32, device="cuda").contiguous()
    H = ctl.value_hessian(x)
    assert ctl._user_hessian_refused and torch.equal(H, vf.value_hessian(x))
    t0 = time.perf_counter()
    assert torch.equal(ctl.value_hessian(x), H)
    with pytest.raises(NotImplementedError, match="scratch"):
        vf.fused_value_hessian(x)
    torch.cuda.synchronize()
    assert time.perf_counter() - t0 < 0.5
