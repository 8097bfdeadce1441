"""GPU tests of hjbx_softpd_value_hessian_f32 (csrc/hjbx_softpd_hessian.hip), of the Python layer above it and of
utils/debug_helper.local_optimal_x on the soft-PD value network.

Yardstick: tests/softhessref.py, the closed form of d2V/dx2 in float64 NumPy, and the same statements in float32 on the CPU (the "CPU float
build").  Errors are taken PER SAMPLE relative to that sample's own max |H_ref|, never a batch-wide scale; max and p99 over the batch must be
within 2 x the same statistic of the CPU float32 evaluation (floor: 2^-24) -- the project's parity rule (README, test_gpu_value_hessian.py).

Networks: lecun-normal kernels from the seeded controller, every bias (b1, b2, b3, b4) seeded uniform(-0.5, 0.5) -- the default zero biases
would leave the bias-initialised accumulators untested -- mean != 0 and std != 1 as in test_gpu_value_hessian.py.  States: x = xf + U(-1, 1) x
box as there (rates capped at 3, angles widened to +-1.25 pi so that they cross the wrap seam); a state within 1e-5 of the seam is left out
(the float32 and float64 wraps may legitimately differ by 2 pi there), at most 2 % may be, which is asserted.  Smooth activations lose nothing
else."""
import json
import os
import types

import numpy as np
import pytest
import torch

from conftest import ANGLE_IDX, ROOT, make_dynamics, make_vhjb_config
from oracle import oracle as O
from softhessref import SoftHessRef
from q_learning_with_hjb_amd import _abi, _ops
from q_learning_with_hjb_amd.controller.vhjb import SoftPDValueFunctionApproximator, VHJBController
from q_learning_with_hjb_amd.utils.debug_helper import local_optimal_x

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
B_FULL = 1000                                   # not a multiple of any C = 32 // n and not of 32
SYSTEMS_H = ["linear", "cartpole", "quad2d", "nearhover"]      # n = 2, 4, 6, 10
ACTS = ["tanh", "sin"]
SENTINEL = 12345.678
EPS_G = 2e-5                                    # the gradient kernel's own parity bound (test_gpu_vhjb.py)

_cases = {}
_report = {}


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    if not _report:
        return
    path = os.path.join(ROOT, "profiles", "softpd_value_hessian.json")
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


def _controller(name, activation, dtype=torch.float32, seed=3):
    d = make_dynamics(name)
    n = d.state_dim
    xf = [float(np.float32(v)) for v in make_vhjb_config(name).xf]
    kw = dict(xf=xf, normalization_mean=[((k % 3) - 1) / 16.0 + 1.0 / 32.0 for k in range(n)],          # all float32 numbers
              normalization_std=[(0.75, 1.5, 1.25, 2.0, 0.5)[k % 5] for k in range(n)])
    ctl = VHJBController(d, make_vhjb_config(name, **kw), dtype=dtype, activation=activation, value_structure="soft_pd")
    vf = ctl.value_function_approximator
    assert isinstance(vf, SoftPDValueFunctionApproximator)
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in vf.parameters():
            if p.dim() == 1:
                p.copy_(torch.rand(p.shape, generator=gen, dtype=torch.float32) - 0.5)       # float32 numbers in either dtype
    return d, ctl


def _states(name, ctl, B, seed):
    box = np.asarray(ctl.obs_max, np.float64).clip(max=3.0)
    box[ANGLE_IDX[name]] = 1.25 * np.pi
    g = torch.Generator(device="cuda").manual_seed(seed)
    u = torch.rand((B, ctl.state_dim), generator=g, device="cuda") * 2 - 1
    xf = torch.as_tensor(np.asarray(ctl.xf, np.float64), dtype=torch.float32, device="cuda")
    return (xf + u * torch.as_tensor(box, dtype=torch.float32, device="cuda")).contiguous()


def _away_from_seam(name, ctl, xr):
    keep = np.ones(xr.shape[0], bool)
    for k in ANGLE_IDX[name]:
        keep &= np.abs(np.abs(xr[:, k] - float(ctl.xf[k])) - np.pi) > 1e-5
    return keep


def _reference(d, vf, activation):
    orc = O.System.from_dynamics(d)
    params = [p.detach().cpu().numpy().astype(np.float64) for p in vf.parameters()]
    return SoftHessRef(params, vf._np["mean"], vf._np["std"], vf._np["xf"], lambda e, dtype: O.wrap(orc, e, dtype=dtype), activation)


def _evaluate(name, ctl, ref, B, seed):
    x = _states(name, ctl, B, seed)
    xr = x.cpu().numpy().astype(np.float64)
    keep = _away_from_seam(name, ctl, xr)
    assert keep.mean() >= 0.98, f"{name}: {1 - keep.mean():.2%} of the states left out"
    return types.SimpleNamespace(x=x, xr=xr, keep=keep, H64=ref.hessian(xr), H32=ref.hessian(xr, dtype=np.float32))


def case(name, activation):
    """One controller, B_FULL states, the float64 and CPU-float32 references: computed once, shared by the tests, never modified."""
    key = (name, activation)
    if key not in _cases:
        d, ctl = _controller(name, activation)
        vf = ctl.value_function_approximator
        ref = _reference(d, vf, activation)
        c = _evaluate(name, ctl, ref, B_FULL, 7 + len(name))
        c.d, c.ctl, c.vf, c.ref = d, ctl, vf, ref
        _cases[key] = c
    return _cases[key]


def _rel_err(got, want):
    """|got - want| / (the sample's max |want|), per element"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = np.abs(want).reshape(want.shape[0], -1).max(1)
    return np.abs(got - want) / scale.reshape((-1,) + (1,) * (want.ndim - 1))


def _stats(err):
    return dict(max=float(err.max()), p99=float(np.quantile(err, 0.99)))


def _parity_line(label, H, c):
    """Prints the figures, then asserts the parity rule; -> the line for the report."""
    sg, sc = _stats(_rel_err(H, c.H64)[c.keep]), _stats(_rel_err(c.H32, c.H64)[c.keep])
    line = dict(kernel=sg, cpu_f32=sc, ratio_max=sg["max"] / max(sc["max"], U), ratio_p99=sg["p99"] / max(sc["p99"], U),
                left_out=float(1 - c.keep.mean()))
    print(f"    {label}: err / sample scale  kernel max {sg['max']:.2e} p99 {sg['p99']:.2e} | CPU float32 max {sc['max']:.2e} "
          f"p99 {sc['p99']:.2e} | kernel / CPU: max {line['ratio_max']:.2f} p99 {line['ratio_p99']:.2f}")
    assert sg["max"] <= 2.0 * max(sc["max"], U), line
    assert sg["p99"] <= 2.0 * max(sc["p99"], U), line
    return line


# ------------------------------------------------------------------------------------------------------------------------------------
# parity
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("activation", ACTS)
@pytest.mark.parametrize("name", SYSTEMS_H)
def test_hessian_vs_f64_closed_form(name, activation):
    c = case(name, activation)
    n = c.ctl.state_dim
    assert c.ctl.fused_value_grad
    # the torch closed form of the module, here in float32, against the restatement: 1e-4 of the sample's scale (five products of up to 128
    # terms and one of 64 deep: (5 x 128 + 64) x 2^-24 = 4.2e-5 as a crude forward bound)
    Ht = c.vf.value_hessian(c.x)
    assert Ht.dtype == torch.float32 and tuple(Ht.shape) == (B_FULL, n, n)
    et = _rel_err(Ht.cpu().numpy(), c.H64)[c.keep].max()
    print(f"    {name} {activation}: torch closed form (float32) err / sample scale max {et:.2e}")
    assert et <= 1e-4, et
    Hk = c.vf.fused_value_hessian(c.x)
    torch.cuda.synchronize()
    assert Hk.shape == (B_FULL, n, n) and Hk.dtype == torch.float32
    H = Hk.cpu().numpy()
    assert np.isfinite(H).all()
    line = _parity_line(f"{name} {activation} H", H, c)
    _report[f"{name}-{activation}"] = line
    # symmetric up to rounding: twice the parity bound of the two elements
    asym = _rel_err(H, H.transpose(0, 2, 1))[c.keep].max()
    asym_cpu = _rel_err(c.H32, c.H32.transpose(0, 2, 1))[c.keep].max()
    print(f"    {name} {activation}: |H - H'| / sample scale max {asym:.2e} (CPU float32 build: {asym_cpu:.2e})")
    assert asym <= 4.0 * max(line["cpu_f32"]["max"], U), asym
    # the controller picks the kernel
    assert torch.equal(c.ctl.value_hessian(c.x), Hk)


# ------------------------------------------------------------------------------------------------------------------------------------
# work distribution: every wave pulls from the LDS counter, partial last tile group, tile edges, rows beyond the batch
# ------------------------------------------------------------------------------------------------------------------------------------
def _raw_call(c, x, B, rows):
    """the entry point on a buffer of `rows` rows pre-filled with a sentinel"""
    n = c.ctl.state_dim
    Hb = torch.full((rows, n, n), SENTINEL, dtype=torch.float32, device="cuda")
    _abi.check(_abi.lib().hjbx_softpd_value_hessian_f32(c.d.system.ptr, _abi.ref(c.vf.descriptor()), x.data_ptr(), Hb.data_ptr(), B,
                                                        torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return Hb


@pytest.mark.parametrize("name, activation", [("linear", "tanh"), ("cartpole", "sin"), ("quad2d", "tanh"), ("nearhover", "sin")])
def test_work_distribution_and_tile_edges(name, activation):
    """B = 6 C (number of CUs) + 1: each workgroup's range holds six tile groups, four taken statically and the rest pulled by its waves from
    the LDS counter, and the last tile group holds one sample.  Same parity bound as at B = 1000.  Then B in {1, C - 1, C, C + 1} into a
    buffer with two more rows: rows >= B keep the sentinel, rows < B equal the large run's bit for bit (a sample's result depends on its own
    state only, not on its place in a tile or on the grid)."""
    base = case(name, activation)
    n = base.ctl.state_dim
    C = 32 // n
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = 6 * C * cus + 1
    c = _evaluate(name, base.ctl, base.ref, B, 31 + n)
    c.d, c.ctl, c.vf = base.d, base.ctl, base.vf
    sentinel = torch.tensor(SENTINEL, dtype=torch.float32).view(torch.int32).item()
    big = _raw_call(c, c.x, B, B + 2)
    assert bool((big[B:].view(torch.int32) == sentinel).all()) and not bool((big[:B].view(torch.int32) == sentinel).any())
    _parity_line(f"{name} {activation} B={B}", big[:B].cpu().numpy(), c)
    for Bs in sorted({1, C - 1, C, C + 1}):
        Hb = _raw_call(c, c.x[:Bs].contiguous(), Bs, Bs + 2)
        assert bool((Hb[Bs:].view(torch.int32) == sentinel).all()), f"B={Bs}: a row beyond the batch was written"
        assert torch.equal(Hb[:Bs], big[:Bs]), f"B={Bs}: rows differ from the large run"


# ------------------------------------------------------------------------------------------------------------------------------------
# exact identities
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, activation", [("cartpole", "tanh"), ("nearhover", "sin")])
def test_exact_identities(name, activation):
    d, ctl = _controller(name, activation)          # a controller of its own: the weights are edited
    vf = ctl.value_function_approximator
    x = case(name, activation).x
    H1, H2 = vf.fused_value_hessian(x), vf.fused_value_hessian(x)
    assert torch.equal(H1, H2) and torch.equal(H1, case(name, activation).vf.fused_value_hessian(x))
    assert float(H1.abs().max()) > 0
    w4, b4 = vf.layers[6], vf.layers[7]
    with torch.no_grad():
        b4.add_(3.25)
        assert torch.equal(vf.fused_value_hessian(x), H1)                    # b4 does not reach any derivative
        w4.mul_(2.0)
        assert torch.equal(vf.fused_value_hessian(x), 2.0 * H1)              # every element is linear in w4; a power of two scales exactly
        w4.zero_()
        assert bool((vf.fused_value_hessian(x) == 0).all())


def test_relu_gives_zeros_on_the_stream():
    d, ctl = _controller("cartpole", "relu")
    vf = ctl.value_function_approximator
    c = types.SimpleNamespace(d=d, ctl=ctl, vf=vf)
    x = case("cartpole", "tanh").x
    Hb = _raw_call(c, x, B_FULL, B_FULL + 2)
    sentinel = torch.tensor(SENTINEL, dtype=torch.float32).view(torch.int32).item()
    assert bool((Hb[:B_FULL] == 0).all()) and bool((Hb[B_FULL:].view(torch.int32) == sentinel).all())
    assert bool((ctl.value_hessian(x) == 0).all()) and bool((vf.value_hessian(x) == 0).all())


def test_float64_controller_takes_the_closed_form():
    d, ctl64 = _controller("linear", "tanh", dtype=torch.float64)
    assert not ctl64.fused_value_grad
    x = torch.rand((16, 2), dtype=torch.float64, device="cuda")
    H = ctl64.value_hessian(x)
    assert H.dtype == torch.float64 and H.shape == (16, 2, 2) and float((H - H.transpose(1, 2)).abs().max()) <= 1e-12 * float(H.abs().max())
    ref = _reference(d, ctl64.value_function_approximator, "tanh")
    assert _rel_err(H.cpu().numpy(), ref.hessian(x.cpu().numpy())).max() <= 1e-12


def test_ops_argument_errors():
    c = case("cartpole", "tanh")
    with pytest.raises(ValueError):
        _ops.softpd_value_hessian(c.d.system, c.vf.descriptor(), c.x[:, :3].contiguous())
    with pytest.raises(ValueError):
        _ops.softpd_value_hessian(c.d.system, c.vf.descriptor(), c.x.double())
    src = ("HJBX_DEV void wrap(T* x) const {}\n"
           "HJBX_DEV void affine(const T* x, T* f1, T* f2) const { for (int i = 0; i < 4; ++i) { f1[i] = x[i]; f2[i] = T(1); } }\n")
    user = _abi.SystemHandle.from_source(_abi.USER_AFFINE, src, 4, 1, 0.02, [-1], [1], [1.0])
    with pytest.raises(NotImplementedError, match="user-defined"):
        _ops.softpd_value_hessian(user, c.vf.descriptor(), c.x)


# ------------------------------------------------------------------------------------------------------------------------------------
# local_optimal_x on the soft-PD network
# ------------------------------------------------------------------------------------------------------------------------------------
def test_local_optimal_x_on_the_soft_pd_network(capsys):
    """Linear system (n = 2), tanh, 256 starts.  A random soft-PD Hessian is indefinite about half the time, so both branches of the helper
    run: x <- x - lr H^-1 dV/dx where det H > 0, x <- x - lr dV/dx elsewhere.  Kept: the starts with cond_2(H64) <= 100 (at least 75 %, at
    least 32 on each side of det H > 0).  One step with lr = 1 against the float64 restatement's step, per start:
        Newton branch:    n cond_2(H64) (eps_H + eps_g) |step64|_inf     (first-order perturbation of a linear solve; eps_H = 2 x the CPU
                          float32 build's max error of this case's parity line, eps_g = 2e-5 the gradient kernel's own parity bound)
        gradient branch:  eps_g max |dV/dx|
    and ten damped steps (lr = 0.1) against the float64 iteration with lr x the same bound, taken at the float64 iterate, summed over the steps."""
    c = case("linear", "tanh")
    ctl, ref, n = c.ctl, c.ref, 2
    first = np.flatnonzero(c.keep)[:256]
    x0 = c.x[torch.as_tensor(first, device="cuda")].contiguous()
    x0r = c.xr[first]
    eps_h = 2.0 * max(_rel_err(c.H32, c.H64)[c.keep].max(), U)

    def step64(x):
        """-> (step, bound, Newton mask) of the float64 restatement at x; as in the helper, a start off the Newton branch solves with I"""
        H, g = ref.hessian(x), ref.grad(x)
        newton = np.linalg.det(H) > 0
        Hs = np.where(newton[:, None, None], H, np.eye(n)[None])
        step = np.linalg.solve(Hs, g[..., None])[..., 0]
        bound = np.where(newton, n * np.linalg.cond(Hs, 2) * (eps_h + EPS_G) * np.abs(step).max(1), EPS_G * np.abs(g).max())
        return step, bound, newton

    s0, b0, newton0 = step64(x0r)
    kept = np.linalg.cond(c.H64[first], 2) <= 100
    with capsys.disabled():          # (the figures go to the terminal, not into the capture the test reads the helper's output from)
        print(f"    starts kept (cond <= 100): {kept.mean():.1%}; Newton branch {int((kept & newton0).sum())}, gradient branch {int((kept & ~newton0).sum())}")
    assert kept.mean() >= 0.75 and (kept & newton0).sum() >= 32 and (kept & ~newton0).sum() >= 32

    x1 = local_optimal_x(x0, ctl, max_iter=1, lr=1.0, verbose=False, newton_method=True)
    assert isinstance(x1, torch.Tensor) and x1.is_cuda and x1.shape == x0.shape and x1.dtype == torch.float32
    err1 = np.abs(x1.cpu().numpy().astype(np.float64) - (x0r - s0)).max(1)
    for label, m in (("Newton", kept & newton0), ("gradient", kept & ~newton0)):
        with capsys.disabled():
            print(f"    one step, {label} branch: max err / bound {float((err1[m] / b0[m]).max()):.3f} over {int(m.sum())} starts")
    assert (err1[kept] <= b0[kept]).all(), float((err1[kept] / b0[kept]).max())

    x10 = local_optimal_x(x0, ctl, max_iter=10, lr=0.1, verbose=True).cpu().numpy().astype(np.float64)
    assert "starts:256" in capsys.readouterr().out
    want, total = x0r.copy(), np.zeros(256)
    for _ in range(10):
        s, b, _ = step64(want)
        want = want - 0.1 * s
        total += 0.1 * b
    err10 = np.abs(x10 - want).max(1)
    with capsys.disabled():
        print(f"    ten damped steps: max err / accumulated bound {float((err10[kept] / total[kept]).max()):.3f}")
    assert (err10[kept] <= total[kept]).all(), float((err10[kept] / total[kept]).max())

    # gradient steps alone
    xg = local_optimal_x(x0, ctl, max_iter=1, lr=1.0, verbose=False, newton_method=False).cpu().numpy().astype(np.float64)
    g0 = ref.grad(x0r)
    assert np.abs(xg - (x0r - g0)).max() <= EPS_G * np.abs(g0).max()
    # container, dtype and rank come back as given: one start as a float64 array (printed per iteration)
    k = int(np.flatnonzero(kept & newton0)[0])
    one = local_optimal_x(x0r[k], ctl, max_iter=1, lr=1.0, verbose=True)
    assert isinstance(one, np.ndarray) and one.shape == (2,) and one.dtype == np.float64 and "iter:0" in capsys.readouterr().out
    assert np.abs(one - (x0r[k] - s0[k])).max() <= b0[k]
