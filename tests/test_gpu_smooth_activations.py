"""GPU tests of the smooth activations (tanh, sin) of the matrix-core kernels ACROSS MAGNITUDES.

The other files evaluate the tanh and sin networks in one regime only: states at 0.5 - 1.5 x the observation box, weights at 1.3 - 1.7 x the
lecun draw, i.e. pre-activations of order one.  A PD network has no biases, so every pre-activation goes to zero as the state approaches
the target -- where a trained controller spends its time -- and a far state drives them past anything a range reduction was written for.

  1. The functions themselves (tanh1, sincos1, relu1 / dact1 of csrc/hjbx_mlp_core.hpp) through hjbx_activation_probe_f32, which runs the
     kernels' own device code over a plain array: ~2^22 arguments per activation, log-uniform in magnitude over every normal binade, both
     signs, plus the edges (+-0, subnormals, thresholds, saturation, k pi/2, inf, NaN), against float64 NumPy on the same float32 inputs.
  2. Every kernel that inlines them -- PD head, soft-PD head, fused rollout, cooperative parameter gradient, the run-time compiled units of
     a user-defined system -- at state scales 1 ... 1e-12 of the box and with weights spread over many binades, judged exactly like the
     existing tanh tests: parity_util.assert_within_cpu_yardstick at the project's factor 2 (value / gradient), the bounds of
     test_value_loss_grad_tanh_network_vs_f64_autograd (parameter gradient), the shape of test_fused_rollout_vs_f64_loop (closed loop).

The targets of these tests are rounded to float32 (`cfg`): the kernels hold xf in float32, the float64 references in float64, and the stock
cart-pole target 3.1415926 is no float32 -- a constant 1e-7 offset in one error coordinate that is invisible at the scale of the box and
IS the error coordinate at 1e-8 of it.  The kernels see the same bits either way."""
import numpy as np
import pytest
import torch

from conftest import ANGLE_IDX, make_dynamics, make_vhjb_config
from netref import smooth_term_scales
from oracle import oracle as O
from parity_util import F32_ULP, abs_err, assert_within_cpu_yardstick, to_np
from q_learning_with_hjb_amd import _abi, _ops
from q_learning_with_hjb_amd.controller.vhjb import VHJBController
from test_gpu_softpd import Restated, error_coords, randomize_biases
from test_gpu_train import _unpack
from test_gpu_vhjb import _autograd_losses, oracle_mlp

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                      # half an ulp of a float32 in [1, 2): the unit of the relative bounds below
SCALES = [1.0, 1e-2, 1e-4, 1e-8, 1e-12]
FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN = float(np.finfo(np.float32).tiny)


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. the functions, through the probe
# ------------------------------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _neighbours(v, k=4):
    """the float32 values within k ulps of v (v > 0)"""
    b = int(_bits(np.array([v], np.float32))[0])
    return np.arange(b - k, b + k + 1, dtype=np.uint32).view(np.float32)


def _log_uniform(rng, count, lo, hi):
    """`count` float32 magnitudes, log-uniform over [lo, hi]: the same number in every binade"""
    m = np.exp2(rng.uniform(np.log2(lo), np.log2(hi), count)).astype(np.float32)
    return np.clip(m, np.float32(lo), np.float32(hi))


def _probe(activation, a):
    h, s = _ops.activation_probe(activation, torch.as_tensor(a, device="cuda"))
    torch.cuda.synchronize()
    return h.cpu().numpy(), s.cpu().numpy()


def test_activation_probe_checks_its_arguments():
    L = _abi.lib()
    a = torch.zeros(8, device="cuda")
    h = torch.full((8,), 7.0, device="cuda")
    assert L.hjbx_activation_probe_f32(3, a.data_ptr(), h.data_ptr(), None, 8, None) == _abi.EINVAL and "unknown activation" in _abi.last_error()
    assert L.hjbx_activation_probe_f32(1, a.data_ptr(), h.data_ptr(), None, -1, None) == _abi.EINVAL
    assert L.hjbx_activation_probe_f32(1, None, h.data_ptr(), None, 8, None) == _abi.EINVAL and "NULL" in _abi.last_error()
    assert L.hjbx_activation_probe_f32(1, a.data_ptr() + 2, h.data_ptr(), None, 4, None) == _abi.EINVAL and "misaligned" in _abi.last_error()
    assert L.hjbx_activation_probe_f32(1, None, None, None, 0, None) == _abi.OK
    assert L.hjbx_activation_probe_f32(1, a.data_ptr(), None, None, 8, None) == _abi.OK
    torch.cuda.synchronize()
    assert bool((h == 7.0).all())                                                  # nothing above wrote anything
    # one output alone, and a size that is no multiple of the workgroup (grid-stride tail): 3 workgroups' worth + 5
    x = torch.linspace(-3, 3, 3 * 256 + 5, device="cuda")
    hh, ss = _ops.activation_probe("tanh", x)
    h2, none = _ops.activation_probe("tanh", x, want_s=False)
    none2, s2 = _ops.activation_probe("tanh", x, want_h=False)
    assert none is None and none2 is None and torch.equal(h2, hh) and torch.equal(s2, ss)
    assert float((hh.double() - torch.tanh(x.double())).abs().max()) < 1e-6


def test_tanh1_relative_error_over_every_binade():
    """tanh1 against float64 tanh on 2^22 arguments, log-uniform over [FLT_MIN, FLT_MAX], both signs, plus the edges.

    ERROR BUDGET of the formula (csrc/hjbx_mlp_core.hpp), in units of u = 2^-24 (a rounding to nearest is <= 1 u relative; v_exp_f32 and
    v_rcp_f32 are 1-ulp operations, <= 2 u relative):
      |x| >= 0.625: t = 1 - 2 q, q = rcp(E + 1), E = exp2(c |x|), c = 2 log2 e.  The argument carries 1 u from its rounding and 0.5 u
          from the rounding of c: E is off by (2 |x| ln 2 / ln 2 = ) 3 |x| u through it, plus 2 u of exp2; E + 1 rounds (1 u); rcp adds 2 u:
              dq / q <= (3 |x| + 2) E / (E + 1) + 3.
          The subtraction turns that into dt / t = (1 - t) / t x dq / q, and the fma rounds once more (1 u).  At x = 0.625: t = 0.5546,
          (1 - t) / t = 0.803, E / (E + 1) = 0.777: 0.803 x (3.875 x 0.777 + 3) + 1 = 5.83 u.  Both factors fall as |x| grows (x = 1: 3.3 u;
          x = 2: 1.4 u), so 6 u bounds this side.
      |x| <  0.625: t = x + x (z P(z)), z = x^2, P the Cephes polynomial (degree 4 in z).  Its approximation error, evaluated in float64 with
          the float32 coefficients, is 0.15 u.  |z P(z)| <= 0.13, evaluated with four fmas and two multiplies (<= 3 u relative, i.e.
          0.13 x 3 / (1 - 0.13) = 0.45 u of the result), and the final fma rounds once (1 u): 1.6 u, asserted as 2 u.
    Asserted: 6 u over the whole normal range (<= the 2^-21 = 8 u the formula was allowed), 2 u below the threshold.
    tanh1 is odd BIT FOR BIT (the exp2 side runs on |x| and copies the sign; the polynomial is odd term by term), +-1 exactly where the
    float32 rounding of float64 tanh is +-1 (the floats around 13 ln 2 are in the sample), NaN for NaN, and the derivative factor
    s = 1 - h^2 (one fma) is within 2 t^2 x (the bound on h) + 1 u of 1 - tanh^2."""
    rng = np.random.default_rng(1)
    mag = np.concatenate([_log_uniform(rng, (1 << 21) - 64, FLT_MIN, FLT_MAX),
                          _neighbours(0.625), _neighbours(13 * np.log(2.0)), _neighbours(1.0),
                          np.array([FLT_MIN, FLT_MAX, 0.0, 1e-45, 1e-40, 5e-39, np.inf, 0.5, 2.0, 9.0, 9.5, 20.0, 44.0, 45.0, 88.0, 89.0], np.float32)])
    a = np.concatenate([mag, -mag, np.array([np.nan], np.float32)]).astype(np.float32)
    h, s = _probe("tanh", a)
    n = mag.size
    assert np.isnan(h[-1]) and np.isnan(s[-1])
    a, h, s = a[:-1], h[:-1], s[:-1]
    t = np.tanh(a.astype(np.float64))
    # odd, bit for bit (+-0 included: the sign of zero is kept)
    assert np.array_equal(_bits(h[:n]) ^ np.uint32(0x80000000), _bits(h[n:]))
    assert _bits(h[a == 0]).tolist() == [0, 0x80000000]
    assert np.all(np.abs(h) <= 1.0) and np.array_equal(h[np.isinf(a)], np.array([1.0, -1.0], np.float32))
    normal = np.isfinite(a) & (np.abs(a) >= FLT_MIN)
    rel = np.abs(h.astype(np.float64) - t)[normal] / np.abs(t[normal])
    small = np.abs(a[normal]) < 0.625
    worst = {k: float(rel[m].max() / U) for k, m in (("below 0.625", small), ("from 0.625", ~small))}
    arg = {k: float(a[normal][m][np.argmax(rel[m])]) for k, m in (("below 0.625", small), ("from 0.625", ~small))}
    print(f"\n    tanh1 max relative error / 2^-24: {worst} at {arg}")
    assert worst["from 0.625"] <= 6.0 and worst["below 0.625"] <= 2.0, (worst, arg)
    # subnormal arguments come back as they are (tanh x = x to far below half an ulp)
    sub = (np.abs(a) < FLT_MIN)
    assert np.array_equal(_bits(h[sub]), _bits(a[sub]))
    # saturation: exactly +-1 only where the correctly rounded float32 tanh is +-1
    sat = np.abs(h) == 1.0
    assert np.all(np.abs(t[sat].astype(np.float32)) == 1.0), a[sat][np.abs(t[sat].astype(np.float32)) != 1.0][:8]
    assert sat[np.abs(a) >= 9.5].all() and not sat[np.abs(a) <= 9.0].any()
    # the derivative factor as the kernels form it: 1 - h^2
    bound = np.where(np.abs(a) < 0.625, 2.0, 6.0) * U
    ds = np.abs(s.astype(np.float64) - (1.0 - t * t))
    ok = np.isfinite(a)
    assert np.all(ds[ok] <= (2.0 * t * t * bound)[ok] + U), float((ds[ok] - (2.0 * t * t * bound)[ok]).max())
    assert np.all(s[ok] >= 0.0) and np.all(s[ok] <= 1.0)


def test_sincos1_accuracy_in_its_domain_and_boundedness_outside():
    """sincos1 against float64 sin / cos.  In the domain |a| <= 1e3 (2^22 arguments log-uniform over [FLT_MIN, 1e3], both signs; 2^20 uniform
    over [-1e3, 1e3], where the error is largest; the multiples k pi/2, |k| <= 636; +-0): absolute error <= 1e-7 for both, the figure
    csrc/hjbx_mlp_core.hpp and DESIGN.md state.  For |a| < 0.78 (k = 0: no reduction, sin = a + a (r^2 P(r^2)) with |r^2 P| <= 0.11
    evaluated to 3 u, polynomial approximation error < 0.5 u, one final rounding) the RELATIVE error of sin is <= 2 x 2^-24, down to the
    smallest normal.  Outside (2^21 arguments log-uniform over [1e3, FLT_MAX], both signs): finite, |sin|, |cos| <= 1 to within one ulp of 1
    (2^-23).  NaN, +inf and -inf give NaN."""
    rng = np.random.default_rng(2)
    mag = np.concatenate([_log_uniform(rng, 1 << 21, FLT_MIN, 1e3), np.array([0.0, 1e3, FLT_MIN, 1e-45, 1e-40], np.float32),
                          (np.arange(0, 637) * (np.pi / 2)).astype(np.float32), _neighbours(np.pi / 4), _neighbours(0.78)])
    a = np.concatenate([mag, -mag, rng.uniform(-1e3, 1e3, 1 << 20).astype(np.float32)])
    assert np.abs(a).max() <= 1e3
    h, s = _probe("sin", a)
    a64 = a.astype(np.float64)
    es, ec = np.abs(h - np.sin(a64)), np.abs(s - np.cos(a64))
    print(f"\n    sincos1 |a| <= 1e3: max abs err sin {es.max():.3e} (a = {a[np.argmax(es)]!r}), cos {ec.max():.3e} (a = {a[np.argmax(ec)]!r})")
    assert es.max() <= 1e-7 and ec.max() <= 1e-7
    k0 = (np.abs(a) < 0.78) & (np.abs(a) >= FLT_MIN)
    rel = es[k0] / np.abs(np.sin(a64[k0]))
    print(f"    sincos1 |a| < 0.78: max relative error of sin / 2^-24: {rel.max() / U:.3f}")
    assert rel.max() <= 2.0 * U
    z = a == 0
    assert z.sum() >= 2 and np.all(h[z] == 0.0) and np.all(s[z] == 1.0)                        # (the reduction gives +0 for -0: r = -0 + 0)
    sub = (np.abs(a) < FLT_MIN) & ~z
    assert np.array_equal(_bits(h[sub]), _bits(a[sub])) and np.all(s[sub] == 1.0)
    # outside the domain: bounded for every finite argument
    far = _log_uniform(rng, 1 << 21, 1e3, FLT_MAX)
    far = np.concatenate([far, np.array([FLT_MAX, 5e7, 1e8, 1e10, 1e13, 2.0 ** 31, 2.0 ** 32, 2.0 ** 63, 2.0 ** 64], np.float32)])
    far = np.concatenate([far, -far])
    h, s = _probe("sin", far)
    assert np.isfinite(h).all() and np.isfinite(s).all()
    print(f"    sincos1 1e3 <= |a| <= FLT_MAX: max |sin| - 1 = {np.abs(h).max() - 1.0:.3e}, max |cos| - 1 = {np.abs(s).max() - 1.0:.3e}")
    assert np.abs(h).max() <= 1.0 + 2.0 ** -23 and np.abs(s).max() <= 1.0 + 2.0 ** -23
    h, s = _probe("sin", np.array([np.nan, np.inf, -np.inf], np.float32))
    assert np.isnan(h).all() and np.isnan(s).all()


def test_relu1_and_its_derivative_factor_are_exact():
    """relu1 is max(a, 0) on the bit pattern: exact for every argument, -0 and every negative value give +0, subnormals pass, +NaN passes.
    The derivative factor is min(max(h x 3e38, 0), 1): exactly 1 for every h with h x 3e38 >= 1 -- every normal h and the subnormals from
    3.4e-39 -- exactly 0 for h <= 0 and for NaN; the subnormals below that get h x 3e38 itself (csrc/hjbx_mlp_core.hpp says "every normal
    h": the ReLU kernels are pinned here as they are)."""
    rng = np.random.default_rng(3)
    mag = np.concatenate([_log_uniform(rng, 1 << 21, FLT_MIN, FLT_MAX),
                          np.array([0.0, FLT_MIN, FLT_MAX, np.inf, 1e-45, 1e-42, 1e-40, 3e-39, 2.0 ** -128, 4e-39, 1.1e-38], np.float32)])
    a = np.concatenate([mag, -mag, np.array([np.nan], np.float32)]).astype(np.float32)
    h, s = _probe("relu", a)
    assert np.isnan(h[-1]) and s[-1] == 0.0
    a, h, s = a[:-1], h[:-1], s[:-1]
    want = np.where(a > 0, a, np.float32(0.0)).astype(np.float32)
    assert np.array_equal(_bits(h), _bits(want))                                     # (bit patterns: -0 -> +0)
    big = want.astype(np.float64) * float(np.float32(3.0e38)) >= 1.0
    assert np.all(s[big] == 1.0) and np.all(s[want == 0] == 0.0)
    tiny = (want > 0) & ~big
    assert tiny.sum() >= 3 and np.all(want[tiny] < 3.4e-39)
    assert np.array_equal(s[tiny], (want[tiny].astype(np.float64) * float(np.float32(3.0e38))).astype(np.float32))


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. the networks' kernels across magnitudes
# ------------------------------------------------------------------------------------------------------------------------------------
def cfg(name, **kw):
    """The stock config of tests/conftest.py with the target rounded to float32 (see the top of the file)."""
    xf = [float(np.float32(v)) for v in make_vhjb_config(name).xf]
    return make_vhjb_config(name, xf=xf, interior_states_mean=xf, boundary_states_mean=xf, **kw)


def controller(name, activation, dtype=torch.float32, dynamics=None, **kw):
    d = make_dynamics(name) if dynamics is None else dynamics
    return d, VHJBController(d, cfg(name), dtype=dtype, activation=activation, **kw)


def states(ctl, B, seed, scale, dtype=torch.float32):
    """xf + scale x box x U(-1, 1) (box: the observation box, its unbounded rate coordinates taken as 3), rounded to float32"""
    rng = np.random.default_rng(seed)
    xf = np.asarray(ctl.xf, np.float64)
    box = np.asarray(ctl.obs_max, np.float64).clip(max=3.0)
    x = torch.as_tensor(xf + scale * box * rng.uniform(-1, 1, (B, xf.size)), dtype=torch.float32, device="cuda").contiguous()
    return x.to(dtype)


def scale_weights(vf, case, activation):
    """The weight cases of test_gpu_vhjb._scale_free_case (applied to the lecun draw, in place) that a smooth activation can take, and a
    saturating one.  sin: layer 1 of "mixed-layers" is scaled by 2^5 instead of 2^20, which keeps the pre-activations inside the documented
    domain of sincos1 (asserted by the caller)."""
    W1, W2, W3 = vf.weights
    with torch.no_grad():
        if case == "tiny-weights":
            W2.mul_(2.0 ** -40); W3.mul_(2.0 ** -30)
        elif case == "mixed-layers":
            W1.mul_(2.0 ** (5 if activation == "sin" else 20)); W2.mul_(2.0 ** -45); W3.mul_(2.0 ** 25)
        elif case == "zero-layer":
            W3.zero_()
        elif case == "saturating":                                  # tanh: most units beyond 13 ln 2, where float32 tanh is exactly 1
            for w in vf.weights:
                w.mul_(8.0)
        elif case == "plain":                                       # the regime of test_tanh_network_fused_kernels_vs_oracle_and_torch
            for w in vf.weights:
                w.mul_(1.7)
        else:
            raise ValueError(case)


def largest_preactivation(W, mean, std, e, activation):
    f = {"tanh": np.tanh, "sin": np.sin}[activation]
    a1 = ((e - np.asarray(mean, np.float64)[None, :]) / np.asarray(std, np.float64)[None, :]) @ W[0]
    a2 = f(a1) @ W[1]
    return max(float(np.abs(a1).max()), float(np.abs(a2).max()))


def judge_pd(label, s, ctl, x, activation):
    """V and dV/dx of the PD head judged as test_tanh_network_fused_kernels_vs_oracle_and_torch judges them: per element against the float64
    oracle, relative to the element's term scale, max and p99.9 within FACTOR = 2 of the oracle's own float32 build (libm tanhf / sinf)."""
    vf = ctl.value_function_approximator
    V, g = vf.fused_value_grad(x)
    assert torch.isfinite(V).all() and torch.isfinite(g).all()
    mlp, W = oracle_mlp(ctl)
    xn = x.cpu().numpy().astype(np.float64)
    oV, og = O.value_grad(s, mlp, *W, xn)
    cV, cg = O.value_grad(s, mlp, *W, xn, dtype=np.float32)
    e = O.wrap(s, xn - np.asarray(vf._np["xf"], np.float64)[None, :])
    if activation == "sin":
        amax = largest_preactivation(W, vf._np["mean"], vf._np["std"], e, activation)
        assert amax <= 1e3, f"{label}: pre-activations up to {amax:.3g} leave the documented domain of sincos1"
    sV, G = smooth_term_scales(W, vf._np["mean"], vf._np["std"], vf.epsilon_scalar, e, activation)
    assert_within_cpu_yardstick(f"{label} V", V.cpu().numpy(), cV, oV, sV)
    assert_within_cpu_yardstick(f"{label} dV/dx", g.cpu().numpy(), cg, og, G)
    return oV


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("name", ["cartpole", "nearhover"])
@pytest.mark.parametrize("activation", ["tanh", "sin"])
def test_pd_value_grad_across_state_scales(activation, name, scale):
    """hjbx_value_grad_f32, B = 1000 (31 tiles + 8), states at xf + scale x box x U(-1, 1): at 1e-2 of the box (a balanced cart-pole) and
    below every pre-activation is small, and V and dV/dx are only as good as the activation is RELATIVE to its own size."""
    d, ctl = controller(name, activation)
    assert ctl.fused_value_grad
    scale_weights(ctl.value_function_approximator, "plain", activation)
    oV = judge_pd(f"{activation} {name} scale {scale:g}", O.System.from_dynamics(d), ctl, states(ctl, 1000, 2, scale), activation)
    assert oV.max() > 0


@pytest.mark.parametrize("case", ["tiny-weights", "mixed-layers", "zero-layer", "saturating"])
@pytest.mark.parametrize("name", ["cartpole", "nearhover"])
@pytest.mark.parametrize("activation", ["tanh", "sin"])
def test_pd_value_grad_across_weight_scales(activation, name, case):
    """hjbx_value_grad_f32 with the weight matrices spread over many binades (test_fused_value_grad_arithmetics_are_scale_free runs these on the
    ReLU network only), B = 1000, states over the whole box."""
    d, ctl = controller(name, activation)
    scale_weights(ctl.value_function_approximator, case, activation)
    judge_pd(f"{activation} {name} {case}", O.System.from_dynamics(d), ctl, states(ctl, 1000, 21, 1.0), activation)


def test_pd_sin_network_stays_bounded_at_far_states():
    """Three coordinates x 1e9 (the "far-states" case of the ReLU tests): the pre-activations are far outside the domain of sincos1, where no
    accuracy is promised -- but |sin| <= 1 for every finite argument, so V and dV/dx are finite and
        V <= (sum |W3|)^2 + eps |e|^2
    (the float32 sum of n squares times eps carries (n + 2) roundings: x (1 + 8 x 2^-24) on that term)."""
    d, ctl = controller("cartpole", "sin")
    vf = ctl.value_function_approximator
    scale_weights(vf, "plain", "sin")
    x = states(ctl, 1000, 21, 1.0)
    x[:, [0, 2, 3]] *= 1e9
    V, g = vf.fused_value_grad(x)
    assert torch.isfinite(V).all() and torch.isfinite(g).all()
    e = O.wrap(O.System.from_dynamics(d), x.cpu().numpy().astype(np.float64) - np.asarray(vf._np["xf"], np.float64)[None, :])
    w3 = float(vf.weights[2].double().abs().sum())
    bound = w3 ** 2 + vf.epsilon_scalar * (e * e).sum(1) * (1.0 + 8 * U)
    Vn = V.double().cpu().numpy()
    assert np.all(Vn >= 0) and np.all(Vn <= bound), float((Vn - bound).max())
    # and what the network adds to eps |e|^2 is really there and really bounded
    net = Vn - vf.epsilon_scalar * (e * e).sum(1)
    assert np.abs(net).max() <= w3 ** 2 + 8 * U * bound.max()


def soft_controller(name, activation, biases):
    from test_gpu_softpd import soft_controller as make
    xf = [float(np.float32(v)) for v in make_vhjb_config(name).xf]
    d, ctl = make(name, activation, cfg_kw=dict(xf=xf, interior_states_mean=xf, boundary_states_mean=xf))
    if biases == "random":
        randomize_biases(ctl.value_function_approximator, 11)
    return d, ctl


def judge_soft(label, d, ctl, x):
    """test_gpu_softpd.test_fused_value_grad_vs_f64_restatement's judgement (float64 `Restated` network; the same in CPU float32 as the
    yardstick), relative to the term scales alone (without that test's absolute floor of 2^-24: V goes to zero with the state here)."""
    vf = ctl.value_function_approximator
    V, g = vf.fused_value_grad(x)
    oV, og, sV, sg, _ = (to_np(t) for t in Restated(vf, torch.float64, "cuda")(error_coords(d, ctl, x, torch.float64)))
    cV, cg, _, _, _ = Restated(vf, torch.float32, "cpu")(error_coords(d, ctl, x, torch.float32).cpu())
    assert_within_cpu_yardstick(f"{label} V", V, cV, oV, sV)
    assert_within_cpu_yardstick(f"{label} gradV", g, cg, og, sg)


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("biases", ["zero", "random"])
@pytest.mark.parametrize("activation", ["tanh", "sin"])
def test_softpd_value_grad_across_state_scales(activation, biases, scale):
    """hjbx_softpd_value_grad_f32 on the cart-pole, B = 1000: with zero biases (the initial network) every layer's pre-activations go to zero
    with the state, three activations deep; with random biases the first layer's stay where the biases put them."""
    d, ctl = soft_controller("cartpole", activation, biases)
    judge_soft(f"soft {activation} {biases} biases scale {scale:g}", d, ctl, states(ctl, 1000, 5, scale))


@pytest.mark.parametrize("B", [1, 31, 33, 65])
@pytest.mark.parametrize("activation", ["tanh", "sin"])
def test_softpd_value_grad_ragged_batches(activation, B):
    """hjbx_softpd_value_grad_f32 below, at and above the 32-environment tile: the entry point was only ever run at B = 2^20 on its own."""
    d, ctl = soft_controller("cartpole", activation, "random")
    x = states(ctl, B, 7, 1.0)
    judge_soft(f"soft {activation} B={B}", d, ctl, x)
    vf = ctl.value_function_approximator
    V, g = vf.fused_value_grad(x)
    big = states(ctl, 97, 8, 1.0)                       # the same rows inside a larger batch: a tile's padding lanes change nothing
    big[:B] = x
    V2, g2 = vf.fused_value_grad(big)
    assert torch.equal(V2[:B], V) and torch.equal(g2[:B], g)


@pytest.fixture(scope="module")
def user_cartpole():
    """One damped cart-pole (a system without a built-in kernel) for this file: its units are compiled once per activation."""
    from test_gpu_user_train import dyn
    return dyn("cartpole_damped")


def user_controller(d, activation, dtype=torch.float32, **kw):
    return VHJBController(d, cfg("cartpole"), dtype=dtype, activation=activation, **kw)


@pytest.mark.parametrize("activation", ["tanh", "sin"])
def test_user_system_value_grad_near_the_target(user_cartpole, activation):
    """The run-time compiled matrix-core unit of a user-defined system (hiprtc compiles csrc/hjbx_mlp_core.hpp under its own flags) at 1e-4 of
    the box, judged like the built-in kernel (the wrap of the damped cart-pole is the cart-pole's: the oracle's network applies)."""
    d = user_cartpole
    ctl = user_controller(d, activation)
    assert d.system.matrix_cores and ctl.fused_value_grad
    scale_weights(ctl.value_function_approximator, "plain", activation)
    s = O.System(_abi.SYS_CARTPOLE, 4, 1, d.dt, d.umin, d.umax, [d.mc, d.mp, d.l, d.g])
    judge_pd(f"user cart-pole {activation} scale 1e-4", s, ctl, states(ctl, 1000, 2, 1e-4), activation)


def test_tanh_closed_loop_from_near_goal_starts():
    """Cart-pole, tanh network, starts at 1e-3 of the box, B = 1024, T = 20: the fused rollout against the oracle's float64 loop in the shape
    of test_gpu_softpd.test_fused_rollout_vs_f64_loop -- at every fifth step the p99 of the state error, relative to the largest error
    coordinate of that step, within 2x of the oracle's float32 loop's, and done_step agreement no worse than that loop's."""
    name, B, T = "cartpole", 1024, 20
    d, ctl = controller(name, "tanh")
    vf = ctl.value_function_approximator
    scale_weights(vf, "plain", "tanh")
    x0 = states(ctl, B, 12, 1e-3)
    ds = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    got = _ops.vhjb_rollout(d.system, ctl._task, vf.descriptor(), x0, T + 1, T, ds)
    mlp, W = oracle_mlp(ctl)
    s = O.System.from_dynamics(d)
    x0n = x0.cpu().numpy().astype(np.float64)
    ref = O.vhjb_rollout(s, ctl._task, mlp, *W, x0n, T)
    c32 = O.vhjb_rollout(s, ctl._task, mlp, *W, x0n, T, dtype=np.float32)
    gt, gds = to_np(got["traj"])[:T + 1], ds.cpu().numpy()
    wt, wds, ct, cds = ref["traj"], ref["done_step"], c32["traj"].astype(np.float64), c32["done_step"]
    assert int((gds != wds).sum()) <= max(int((cds != wds).sum()), B // 1000)
    live_all = (gds == wds) & (cds == wds)
    xf = np.asarray(ctl.xf, np.float64)
    checked = 0
    for t in range(1, T + 1, 5):
        keep = live_all & (wds > t)
        assert keep.sum() >= 100
        scale = np.abs(O.wrap(s, wt[t] - xf[None, :])).max()
        eg = abs_err(gt[t], wt[t], ANGLE_IDX[name])[keep] / scale
        ec = abs_err(ct[t], wt[t], ANGLE_IDX[name])[keep] / scale
        pg, pc = float(np.quantile(eg, 0.99)), float(np.quantile(ec, 0.99))
        print(f"    tanh {name} step {t}: |e| up to {scale:.2e}; p99 err / scale kernel {pg:.2e} CPU float32 {pc:.2e}")
        assert pg <= 2.0 * max(pc, F32_ULP), (t, pg, pc)
        checked += 1
    assert checked == 4


def reference_sums(make64, ctl32, xs, dones, costs, mode):
    """test_gpu_train._reference_sums_f64 for a controller built by `make64(mode)` (float64, this file's config): float64 autograd double
    back-prop of the loss SUMS on the float32 weights -> (g_h list, g_t list, scalars)."""
    ctl64 = make64(mode)
    with torch.no_grad():
        for w64, w32 in zip(ctl64.value_function_approximator.weights, ctl32.value_function_approximator.weights):
            w64.copy_(w32.double())
    x64, dn64, c64 = xs.double(), dones.double(), costs.double()
    params = list(ctl64.value_function_approximator.parameters())
    if mode == _abi.RESIDUAL_NORMALISED:
        h, t = _autograd_losses(ctl64, x64, dn64, c64)
        n_int, n_done = float((1 - dn64).sum()), float(dn64.sum())
        hs, ts = h * (n_int + ctl64.epsilon), t * (n_done + ctl64.epsilon)
    else:
        hs, hsums = ctl64._hjb_sums(x64, dn64)
        ts, _ = ctl64._termination_sums(x64, dn64, c64)
        n_int, n_done = float(hsums[1]), float(hsums[2])
    g_h = torch.autograd.grad(hs, params, retain_graph=True, allow_unused=True)
    g_t = torch.autograd.grad(ts, params, allow_unused=True)
    z = lambda g, p: torch.zeros_like(p) if g is None else g
    return [z(g, p) for g, p in zip(g_h, params)], [z(g, p) for g, p in zip(g_t, params)], (float(hs), float(ts), n_int, n_done)


def minibatch(ctl, B, seed, scale):
    xs = states(ctl, B, seed, scale)
    rng = np.random.default_rng(seed + 100)
    dones = torch.as_tensor((rng.uniform(size=B) < 0.3).astype(np.float32), device="cuda")
    costs = torch.as_tensor(rng.uniform(0.5, 20, B).astype(np.float32), device="cuda")
    return xs, dones, costs


def judge_param_grad(label, d, ctl, make64, xs, dones, costs, mode):
    """The bounds of test_gpu_train.test_value_loss_grad_tanh_network_vs_f64_autograd: counts exact, loss sums to 2e-5, every gradient matrix
    to 1e-4 of its largest entry per element and 1e-4 in the Frobenius norm."""
    vf = ctl.value_function_approximator
    flat = _ops.value_loss_grad(d.system, ctl._task, vf.descriptor(), xs, costs, dones, mode=mode)
    gh, gt, sc = _unpack(flat, d.state_dim)
    rh, rt, rsc = reference_sums(make64, ctl, xs, dones, costs, mode)
    assert sc[2] == rsc[2] and sc[3] == rsc[3]
    assert abs(sc[0] - rsc[0]) <= 2e-5 * abs(rsc[0]) + 1e-6 and abs(sc[1] - rsc[1]) <= 2e-5 * abs(rsc[1]) + 1e-6, (sc, rsc)
    lines, bad = [], []
    for which, got, want in (("hjb", gh, rh), ("termination", gt, rt)):
        for k, (a, b) in enumerate(zip(got, want)):
            b = b.cpu().numpy()
            scale = np.abs(b).max()
            assert scale > 0
            rmax, rfro = np.abs(a - b).max() / scale, np.linalg.norm(a - b) / np.linalg.norm(b)
            lines.append(f"{which} dW{k + 1}: max {rmax:.2e} Frobenius {rfro:.2e}")
            if rmax > 1e-4 or rfro > 1e-4:
                bad.append(lines[-1])
    print(f"    {label}: err / scale per matrix: " + "; ".join(lines))
    assert not bad, f"{label}: {bad}"


@pytest.mark.parametrize("mode", [_abi.RESIDUAL_NORMALISED, _abi.RESIDUAL_RAW])
@pytest.mark.parametrize("B", [33, 256])
@pytest.mark.parametrize("scale", [1e-2, 1e-4])
@pytest.mark.parametrize("activation", ["tanh", "sin"])
def test_value_loss_grad_near_the_target(activation, scale, B, mode):
    """hjbx_value_loss_grad_f32 (cooperative kernel; cart-pole, n = 4) on minibatches drawn at 1e-2 and 1e-4 of the box: the second-order
    sweep multiplies by h (tanh) and by 1 - h^2, so it sees the activation's relative error too."""
    d, ctl = controller("cartpole", activation, residual_mode=mode)
    assert ctl.fused_param_grad
    with torch.no_grad():
        for w in ctl.value_function_approximator.weights:
            w.mul_(1.5)
    xs, dones, costs = minibatch(ctl, B, 41, scale)
    make64 = lambda m: controller("cartpole", activation, torch.float64, residual_mode=m)[1]
    judge_param_grad(f"{activation} scale {scale:g} B={B} mode {mode}", d, ctl, make64, xs, dones, costs, mode)


def test_user_system_value_loss_grad_near_the_target(user_cartpole):
    """The same through the run-time compiled parameter-gradient unit of a user-defined system (tanh, 1e-4 of the box, B = 256)."""
    d = user_cartpole
    ctl = user_controller(d, "tanh")
    assert ctl.fused_param_grad
    with torch.no_grad():
        for w in ctl.value_function_approximator.weights:
            w.mul_(1.5)
    xs, dones, costs = minibatch(ctl, 256, 41, 1e-4)
    make64 = lambda m: user_controller(d, "tanh", torch.float64, residual_mode=m)
    judge_param_grad("user cart-pole tanh scale 1e-4 B=256", d, ctl, make64, xs, dones, costs, _abi.RESIDUAL_NORMALISED)
