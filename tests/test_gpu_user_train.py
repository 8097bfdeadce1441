"""GPU tests of the fused parameter gradient for user-defined systems: hjbx_value_loss_grad_f32 / hjbx_value_loss_adam_f32 on a handle with
the matrix-core kernels enabled run k_train_coop compiled at run time for the user's struct (csrc/hjbx_user_train_kernels.hpp), followed
by the library's own reduce / update epilogue.

  * the flat gradient buffer of the damped cart-pole (no built-in twin) and of the user planar quadrotor against the float64 autograd
    double back-prop restatement of tests/test_gpu_train.py on the same float32 weights, with that file's bounds; the user quadrotor's
    Frobenius error per matrix is also held to 2 x the built-in quad2d kernel's on the same inputs (the project's yardstick factor);
  * size-independent properties at B = 2^17; hjbx_value_loss_adam_f32 step for step; the fused-epilogue argument checks happen before the
    first launch (built-in and user path alike);
  * the controller: fused_param_grad for such a system, the device-driven fit phase bit-equal to the per-minibatch loop, agreement with the
    autograd path, the graphed update, and the autograd fall-back with one warning when the library refuses the unit.
Dynamics objects are shared between the tests of a process: a unit is compiled once per system and activation."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest
import torch

from conftest import make_vhjb_config
from q_learning_with_hjb_amd import _abi, _ops
from q_learning_with_hjb_amd.configs import defaults as D
from q_learning_with_hjb_amd.controller.vhjb import VHJBController, adam_state
from q_learning_with_hjb_amd.dynamics.quadrotors import Quadrotors2D
from test_gpu_train import _batch, _mixed_grads, _unpack
from test_gpu_vhjb import _autograd_losses, states_near_target
from test_user_fused_host import fused_systems
from test_user_train_host import train_systems

pytestmark = pytest.mark.gpu

CONFIG = {"cartpole_damped": "cartpole", "quad2d": "quad2d", "manip10": "nearhover"}


@functools.lru_cache(maxsize=None)
def dyn(name):
    return train_systems()[name]()        # (param_grad=True in device_source(): the controller fuses the parameter gradient by default)


def controller(name, dtype=torch.float32, cfg=None, **kw):
    d = dyn(name)
    return d, VHJBController(d, make_vhjb_config(CONFIG[name], **(cfg or {})), dtype=dtype, **kw)


def _reference_sums(name, ctl32, xs, dones, costs, mode, dtype=torch.float64):
    """tests/test_gpu_train.py::_reference_sums_f64 on a controller of the USER system: autograd double back-prop of the loss sums on the
    float32 weights, in float64 (the reference) or float32 (PyTorch's own float32 evaluation)."""
    kw = dict(fused_param_grad=False) if dtype == torch.float32 else {}
    _, ctl64 = controller(name, dtype, residual_mode=mode, activation=ctl32.value_function_approximator.activation, **kw)
    with torch.no_grad():
        for w64, w32 in zip(ctl64.value_function_approximator.weights, ctl32.value_function_approximator.weights):
            w64.copy_(w32.to(dtype))
    x64, dn64, c64 = xs.to(dtype), dones.to(dtype), costs.to(dtype)
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


@pytest.mark.parametrize("B", [1, 33, 256, 1000])
@pytest.mark.parametrize("mode", [_abi.RESIDUAL_NORMALISED, _abi.RESIDUAL_RAW])
@pytest.mark.parametrize("activation", ["relu", "tanh"])
@pytest.mark.parametrize("name", ["cartpole_damped", "quad2d"])
def test_user_value_loss_grad_vs_f64_autograd(name, activation, mode, B):
    """The run-time compiled kernel vs float64 autograd double back-prop on a float64 controller of the user system: every gradient matrix
    to 1e-4 of its largest entry per element and 1e-4 in the Frobenius norm, loss sums to 1e-5, counts exact (the bounds of
    tests/test_gpu_train.py).  The user quadrotor in addition: Frobenius error per matrix <= 2 x that of the built-in quad2d kernel on the
    same inputs and weights against the same reference (floor 2^-23 of the matrix norm under the denominator; bit-equality is not
    required: the two evaluate the dynamics with different expressions)."""
    d, ctl = controller(name, activation=activation, residual_mode=mode)
    assert ctl.fused_param_grad
    vf = ctl.value_function_approximator
    with torch.no_grad():
        for w in vf.weights:
            w.mul_(1.3)
    xs, dones, costs = _batch(d, ctl, B, 31)
    flat = _ops.value_loss_grad(d.system, ctl._task, vf.descriptor(), xs, costs, dones, mode=mode)
    torch.cuda.synchronize()
    gh, gt, sc = _unpack(flat, d.state_dim)
    rh, rt, rsc = _reference_sums(name, ctl, xs, dones, costs, mode)
    twin = None
    if name == "quad2d":
        db = Quadrotors2D(D.quadrotors2d_dynamics_config())
        twin = _unpack(_ops.value_loss_grad(db.system, ctl._task, vf.descriptor(), xs, costs, dones, mode=mode), d.state_dim)
    print(f"\n    {name} {activation} mode {mode} B={B}: sums {sc[0]:.6e} / {rsc[0]:.6e}, {sc[1]:.6e} / {rsc[1]:.6e}")
    assert sc[2] == rsc[2] and sc[3] == rsc[3]
    assert abs(sc[0] - rsc[0]) <= 1e-5 * abs(rsc[0]) + 1e-6 and abs(sc[1] - rsc[1]) <= 1e-5 * abs(rsc[1]) + 1e-6, (sc, rsc)
    for s, (label, got, want) in enumerate((("hjb", gh, rh), ("termination", gt, rt))):
        for k, (a, b) in enumerate(zip(got, want)):
            b = b.cpu().numpy()
            scale = np.abs(b).max()
            if scale == 0:
                assert np.abs(a).max() == 0
                continue
            err, fro, nb = np.abs(a - b), np.linalg.norm(a - b), np.linalg.norm(b)
            line = f"    {label} dW{k + 1}: max err / scale {err.max() / scale:.2e}, Frobenius rel {fro / nb:.2e}"
            if twin is not None:
                fro_twin = np.linalg.norm(twin[s][k] - b)
                line += f", built-in twin {fro_twin / nb:.2e}, ratio {fro / max(fro_twin, 2.0 ** -23 * nb):.2f}"
            print(line)
            assert err.max() <= 1e-4 * scale, f"{label} dW{k + 1}: max err {err.max():.3e} vs scale {scale:.3e} (rel {err.max() / scale:.2e})"
            assert fro <= 1e-4 * nb, f"{label} dW{k + 1}: Frobenius rel {fro / nb:.2e}"
            if twin is not None:
                assert fro <= 2.0 * max(fro_twin, 2.0 ** -23 * nb), f"{label} dW{k + 1}: Frobenius error {fro:.3e} vs built-in twin {fro_twin:.3e}"


def test_user_value_loss_grad_properties_at_scale():
    """User quadrotor, B = 2^17 (more tiles than workgroups): (a) two launches are bit-identical, also when the workspace is handed over
    full of garbage (nothing has to be initialised between launches), (b) additive over a split of the batch -- the parts have ragged
    tails, i.e. padding lanes -- to the tolerance of tests/test_gpu_train.py, (c) done samples contribute nothing to the hjb set and only
    they contribute to the termination set."""
    d, ctl = controller("quad2d")
    vf = ctl.value_function_approximator
    B = 1 << 17
    xs, dones, costs = _batch(d, ctl, B, 9, frac=0.8)
    n = d.state_dim
    P = n * 128 + 128 * 128 + 128 * 64
    call = lambda sl: _ops.value_loss_grad(d.system, ctl._task, vf.descriptor(), xs[sl].contiguous(), costs[sl].contiguous(), dones[sl].contiguous())
    full = call(slice(None))
    again = call(slice(None))
    assert torch.equal(full, again)
    ws = torch.full((int(_abi.lib().hjbx_value_loss_grad_workspace_bytes(B)),), 0xFF, dtype=torch.uint8, device="cuda")       # (NaN patterns)
    third = torch.empty_like(full)
    _abi.check(_abi.lib().hjbx_value_loss_grad_f32(d.system.ptr, _abi.ref(ctl._task), _abi.ref(vf.descriptor()), ctl.residual_mode, xs.data_ptr(),
                                                   costs.data_ptr(), dones.data_ptr(), third.data_ptr(), ws.data_ptr(), B, None))
    _abi.check(_abi.lib().hjbx_value_loss_grad_f32(d.system.ptr, _abi.ref(ctl._task), _abi.ref(vf.descriptor()), ctl.residual_mode, xs.data_ptr(),
                                                   costs.data_ptr(), dones.data_ptr(), third.data_ptr(), ws.data_ptr(), B, None))   # ... and used again as it is
    torch.cuda.synchronize()
    assert torch.equal(full, third)
    k = 50011
    parts = call(slice(0, k)).double() + call(slice(k, B)).double()
    err = (full.double() - parts).abs()
    scale = torch.stack([full[:P].abs().max(), full[P:2 * P].abs().max()]).double()
    assert float(err[:P].max()) <= 2e-5 * float(scale[0]) and float(err[P:2 * P].max()) <= 2e-5 * float(scale[1])
    assert float(err[2 * P:2 * P + 2].max()) <= 1e-5 * float(full[2 * P:2 * P + 2].abs().max())
    assert torch.equal(full[2 * P + 2:], parts[2 * P + 2:].float())            # the counts are exact
    assert float(full[2 * P + 2] + full[2 * P + 3]) == B
    live = dones == 0
    only_live = _ops.value_loss_grad(d.system, ctl._task, vf.descriptor(), xs[live].contiguous(), costs[live].contiguous(), dones[live].contiguous())
    assert float(only_live[P:2 * P].abs().max()) == 0.0 and float(only_live[2 * P + 1]) == 0.0
    assert float((only_live[:P].double() - full[:P].double()).abs().max()) <= 2e-5 * float(scale[0])


@pytest.mark.parametrize("name,activation", [("cartpole_damped", "relu"), ("quad2d", "tanh"), ("cartpole_damped", "sin")])
def test_user_value_loss_adam_step_for_step(name, activation):
    """hjbx_value_loss_adam_f32 on a user system, three steps: (a) == hjbx_value_loss_grad_f32 + hjbx_mix_adam_f32 bit for bit (the same sums
    in the same order: the assertion of the built-in test), and (b) against hjbx_value_loss_grad_f32 + hjbx_mix_gradients_f32 +
    torch.optim.Adam with the tolerances of test_mix_adam_follows_torch_adam_step_for_step."""
    d, ctl = controller(name, activation=activation)
    vf = ctl.value_function_approximator
    xs, dones, costs = _batch(d, ctl, 300, 13)
    lr, b1, b2, eps_adam = 1e-3, 0.9, 0.999, 1e-8
    state = []
    for fused in (True, False):
        w = [p.detach().clone().contiguous() for p in vf.parameters()]
        m, v = [torch.zeros_like(p) for p in w], [torch.zeros_like(p) for p in w]
        steps = [torch.zeros((), device="cuda") for _ in w]
        ticket, acc, counter = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(3, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
        desc = vf.descriptor()
        desc.W1, desc.W2, desc.W3 = (t.data_ptr() for t in w)
        theirs = [torch.nn.Parameter(p.clone()) for p in w]
        opt = torch.optim.Adam(theirs, lr=lr, betas=(b1, b2), eps=eps_adam)
        out = []
        for it in range(3):
            reg = 0.2 * (it + 1)
            if fused:
                # torch.optim.Adam on the mixed gradient of the same flat buffer, evaluated at the library's weights of this step
                flat = _ops.value_loss_grad(d.system, ctl._task, desc, xs, costs, dones, mode=ctl.residual_mode)
                mixed, _ = _ops.mix_gradients(flat, sum(p.numel() for p in w), reg, ctl.epsilon)
                off = 0
                for p in theirs:
                    p.grad = mixed[off:off + p.numel()].view_as(p).clone()
                    off += p.numel()
                opt.step()
                losses = _ops.value_loss_adam(d.system, ctl._task, desc, xs, costs, dones, ctl.residual_mode, reg, ctl.epsilon, w, m, v, steps, ticket, lr, b1, b2,
                                              eps_adam, acc, counter)
                for ours, p, mm, vv in zip(w, theirs, m, v):
                    st = opt.state[p]
                    assert torch.allclose(mm, st["exp_avg"], rtol=1e-5, atol=1e-9) and torch.allclose(vv, st["exp_avg_sq"], rtol=1e-5, atol=1e-12)
                    assert (ours - p).abs().max().item() <= 2e-6 * lr * (it + 1) + 1e-7 * p.abs().max().item()
                    with torch.no_grad():
                        p.copy_(ours)                                   # the next step's gradient is taken at the library's weights
            else:
                flat = _ops.value_loss_grad(d.system, ctl._task, desc, xs, costs, dones, mode=ctl.residual_mode)
                losses = _ops.mix_adam(flat, reg, ctl.epsilon, w, m, v, steps, ticket, lr, b1, b2, eps_adam, acc, counter)
            out.append(losses.clone())
        torch.cuda.synchronize()
        state.append((w, m, v, steps, acc, counter, out, ticket))
    a, b = state
    assert int(a[5]) == int(b[5]) == 3 and int(a[7]) == int(b[7]) == 0 and all(float(x) == float(y) == 3.0 for x, y in zip(a[3], b[3]))
    for k in (0, 1, 2):
        for ta, tb in zip(a[k], b[k]):
            assert torch.equal(ta, tb), (k, float((ta - tb).abs().max()))
    assert torch.equal(a[4], b[4]) and all(torch.equal(x, y) for x, y in zip(a[6], b[6]))
    assert all(float((p - q).abs().max()) > 0 for p, q in zip(a[0], vf.parameters()))              # the weights did move


@pytest.mark.parametrize("user", [True, False])
def test_fuse_arguments_are_checked_before_anything_is_launched(user):
    """Adam tensors of the wrong shapes (the right total): HJBX_EINVAL, and the workspace -- the loss-sum records included -- keeps the
    pattern it was handed over with: no gradient kernel was enqueued.  User path and built-in path alike."""
    if user:
        d, ctl = controller("quad2d", graph_updates=False)
    else:
        from test_gpu_vhjb import controller as builtin_controller
        d, ctl = builtin_controller("cartpole", graph_updates=False)
    vf = ctl.value_function_approximator
    xs, dones, costs = _batch(d, ctl, 256, 3)
    params = [p.data for p in vf.parameters()]
    m, v, steps = adam_state(ctl.optimizer, list(vf.parameters()))
    ticket = torch.zeros(1, dtype=torch.int32, device="cuda")
    st = _ops._adam_struct(params, m, v, steps, ticket, 1e-3, 0.9, 0.999, 1e-8)
    st.numel[0] += 64
    st.numel[1] -= 64
    nbytes = int(_abi.lib().hjbx_value_loss_adam_workspace_bytes(256))
    ws = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device="cuda")
    before = [p.clone() for p in params]
    losses = torch.full((3,), -7.0, device="cuda")
    rc = _abi.lib().hjbx_value_loss_adam_f32(d.system.ptr, _abi.ref(ctl._task), _abi.ref(vf.descriptor()), ctl.residual_mode, xs.data_ptr(), costs.data_ptr(),
                                             dones.data_ptr(), None, 0.1, ctl.epsilon, C.byref(st), losses.data_ptr(), None, None, None, ws.data_ptr(), 256, None)
    torch.cuda.synchronize()
    assert rc == _abi.EINVAL and "Adam state's tensors" in _abi.last_error()
    assert bool((ws == 0x5A).all()) and bool((losses == -7.0).all()) and all(torch.equal(p, q) for p, q in zip(params, before))
    # and the valid call on the same buffers works
    st = _ops._adam_struct(params, m, v, steps, ticket, 1e-3, 0.9, 0.999, 1e-8)
    rc = _abi.lib().hjbx_value_loss_adam_f32(d.system.ptr, _abi.ref(ctl._task), _abi.ref(vf.descriptor()), ctl.residual_mode, xs.data_ptr(), costs.data_ptr(),
                                             dones.data_ptr(), None, 0.1, ctl.epsilon, C.byref(st), losses.data_ptr(), None, None, None, ws.data_ptr(), 256, None)
    torch.cuda.synchronize()
    assert rc == _abi.OK and torch.isfinite(losses).all() and not bool((ws == 0x5A).all())


@pytest.mark.parametrize("name,activation,batch", [("cartpole_damped", "relu", 64), ("quad2d", "tanh", 16)])
def test_user_device_driven_fit_phase_equals_the_per_minibatch_loop(name, activation, batch):
    """VHJBController on an enabled user system reports fused_param_grad, and three epochs of train() with the device-driven fit phase (one
    captured graph per update) are BIT-EQUAL to the per-minibatch loop on eager launches: the assertion of
    tests/test_gpu_train_loop.py::test_device_driven_fit_phase_equals_the_per_minibatch_loop with the library's Adam."""
    import os
    if os.environ.get("HJBX_FUSED_PARAM_GRAD", "1") == "0" or os.environ.get("HJBX_FUSED_ADAM", "1") == "0":
        pytest.skip("the device-driven fit phase belongs to the fused parameter gradient with the library's Adam step")
    kw = dict(epochs=3, num_of_trajectories_per_epoch=5, maximum_step=40, batch_size=batch, maximum_buffer_size=700,
              regularization_warmup_steps_per_cycle=4, regularization_total_steps_per_cycle=9, regularization_num_of_cycles=2, regularization_peak_value=1e-2)
    outs, ctls = [], []
    for graphed in (True, False):
        d = train_systems()[name]()                                  # (a Dynamics object of its own per run, like the built-in test)
        ctl = VHJBController(d, make_vhjb_config(CONFIG[name], **kw), dtype=torch.float32, graph_updates=graphed, activation=activation)
        assert ctl.fused_param_grad is True and ctl.fused_value_grad and ctl._native_adam and ctl._fit_graph_usable() == graphed
        outs.append(ctl.train())
        ctls.append(ctl)
    a, b = ctls
    assert a._fit_graph is not None and a._graphed_update is None and b._fit_graph is None      # the device-driven path did run
    assert a.update_counter == b.update_counter > 3 and a.regularization == b.regularization
    assert len(a.replay_buffer) == len(b.replay_buffer)
    for wa, wb in zip(a.value_function_approximator.weights, b.value_function_approximator.weights):
        assert torch.equal(wa, wb)
    for pa, pb in zip(a.value_function_approximator.parameters(), b.value_function_approximator.parameters()):
        sa, sb = a.optimizer.state[pa], b.optimizer.state[pb]
        assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]) and float(sa["step"]) == float(sb["step"])
    for la, lb in zip(outs[0], outs[1]):
        np.testing.assert_allclose(la, lb, rtol=2e-6)


def test_user_fused_and_autograd_updates_agree():
    """Six updates of the damped cart-pole's controller through the fused kernels against PyTorch autograd + the run-time compiled residual
    kernel, both from the same start and on the same six minibatches, NOT re-synchronised in between; then the weights are compared.

    Bounds.  tests/test_gpu_train.py::test_fused_and_autograd_updates_agree allows the parameter change of ONE Adam step to differ by 1e-6
    where |g| > 1e-5 (away from Adam's eps), the losses by 1e-5 and the mixed gradient by 1e-4 of its largest entry.  Over six steps:
      * every entry: |w_fused - w_autograd| <= 2 x 6 x lr x 1.05.  An Adam step is at most lr |m_hat| / sqrt(v_hat) <= lr in the first steps
        from a zero state (Cauchy-Schwarz over the six bias-corrected weights gives 1.016 lr at t = 6; 1.05 covers it), so two trajectories cannot be further apart, whatever
        the gradients do at the kinks of the loss (|r| at r = 0, the clip of u, the ReLU units);
      * the entries whose autograd gradient stayed away from Adam's eps (|g| > 1e-5) in all six updates: 6 x 1e-6, the one-step tolerance
        times the number of steps -- asserted for their 99th percentile and printed for their maximum (a sample that sits on a kink can be
        taken on different sides by the two float32 evaluations once the weights differ in the last bits, and moves single entries by more);
      * the first update, from identical weights: losses, gradient and parameter change to that test's own tolerances."""
    d, fused = controller("cartpole_damped", fused_param_grad=True, graph_updates=False)
    _, plain = controller("cartpole_damped", fused_param_grad=False, graph_updates=False)
    assert fused.fused_param_grad and not plain.fused_param_grad
    pf, pp = list(fused.value_function_approximator.parameters()), list(plain.value_function_approximator.parameters())
    assert all(torch.equal(a, b) for a, b in zip(pf, pp))
    lr = float(fused.optimizer.param_groups[0]["lr"])
    start = [p.detach().clone() for p in pf]
    away = [torch.ones_like(p, dtype=torch.bool) for p in pf]
    for k in range(6):
        xs, dones, costs = _batch(d, fused, 256, 3 + k)
        gf = _mixed_grads(fused, xs, dones, costs, 0.37) if k == 0 else None
        lf = [float(v) for v in fused.params_update(xs, dones, costs, 0.37)]
        lp = [float(v) for v in plain.params_update(xs, dones, costs, 0.37)]
        gp = [p.grad.detach().clone() for p in pp]
        away = [m & (g.abs() > 1e-5) for m, g in zip(away, gp)]
        rel = max(abs(x - y) / (abs(y) + 1e-30) for x, y in zip(lf, lp))
        print(f"\n    update {k}: losses fused {lf} autograd {lp} (max rel diff {rel:.2e})")
        if k == 0:
            for x, y in zip(lf, lp):
                assert abs(x - y) <= 1e-5 * abs(y) + 1e-7, (lf, lp)
            for ga, gb in zip(gf, gp):
                assert float((ga - gb).abs().max()) <= 1e-4 * float(gb.abs().max())
            for a, b, s0, gb in zip(pf, pp, start, gp):
                big = gb.abs() > 1e-5
                assert float(((a.detach() - s0) - (b.detach() - s0))[big].abs().max()) <= 1e-6
    for i, (a, b, s0, m) in enumerate(zip(pf, pp, start, away)):
        diff = (a.detach() - b.detach()).abs()
        moved = float((a.detach() - s0).abs().max())
        q99 = float(torch.quantile(diff[m].double().flatten()[:1 << 24], 0.99)) if int(m.sum()) else 0.0
        print(f"    W{i + 1} after six updates: max |dw| {float(diff.max()):.3e}, median {float(diff.median()):.3e}; entries away from eps in all six "
              f"({float(m.double().mean()):.1%}): max {float(diff[m].max()) if int(m.sum()) else 0.0:.3e}, q99 {q99:.3e}; moved by {moved:.3e}; lr {lr:g}")
        assert moved > lr                                              # six Adam steps really happened
        assert float(diff.max()) <= 2 * 6 * lr * 1.05
        assert q99 <= 6e-6


def test_user_graphed_update_equals_eager_update():
    """tests/test_gpu_vhjb.py::test_graphed_update_equals_eager_update (float32 row) on the user quadrotor: six optimiser steps replayed from a
    captured graph walk the trajectory of six eager ones -- losses to 1e-4, weights to rtol 2e-3 / atol 2e-5, that test's tolerances."""
    d, a = controller("quad2d")
    _, b = controller("quad2d")
    assert a.fused_param_grad and b.fused_param_grad and a.graph_updates
    pa, pb = list(a.value_function_approximator.parameters()), list(b.value_function_approximator.parameters())
    assert all(torch.equal(x, y) for x, y in zip(pa, pb))
    rng = np.random.default_rng(4)
    B = 256
    start = [p.detach().clone() for p in pa]
    for k in range(6):
        xs = states_near_target(d, a, B, 20 + k, 0.6)
        dones = torch.as_tensor((rng.uniform(size=B) < 0.3).astype(np.float32), device="cuda")
        costs = torch.as_tensor(rng.uniform(0.5, 20, B).astype(np.float32), device="cuda")
        reg = 1e-5 * k
        la = [float(v) for v in a.params_update_graphed(xs, dones, costs, reg)]
        if k == 0:   # the capture itself must not have stepped: after ONE replayed step the weights moved by at most lr
            assert all(float((p - s).abs().max()) <= 1.0001 * float(a.optimizer.param_groups[0]["lr"]) for p, s in zip(pa, start))
        lb = [float(v) for v in b.params_update(xs, dones, costs, reg)]
        np.testing.assert_allclose(la, lb, rtol=1e-4)
    for x, y in zip(pa, pb):
        np.testing.assert_allclose(x.detach().cpu().numpy(), y.detach().cpu().numpy(), rtol=2e-3, atol=2e-5)
    assert all(float((p - s).abs().max()) > 1e-3 for p, s in zip(pa, start))


def test_controller_fuses_when_the_system_or_the_caller_asks():
    """param_grad=True in device_source() makes the automatic mode fuse; a system with matrix_cores=True alone keeps autograd by default (its
    behaviour before this kernel existed) and fuses with fused_param_grad=True; the two fused controllers compute the same gradient."""
    d, ctl = controller("cartpole_damped")
    assert d.system.param_grad and ctl.fused_param_grad is True
    quiet = fused_systems()["cartpole_damped"]()
    cfg = make_vhjb_config("cartpole")
    auto = VHJBController(quiet, cfg, dtype=torch.float32)
    asked = VHJBController(quiet, cfg, dtype=torch.float32, fused_param_grad=True)
    assert not quiet.system.param_grad and auto.fused_param_grad is False and asked.fused_param_grad is True
    xs, dones, costs = _batch(d, ctl, 256, 7)
    with torch.no_grad():
        for a, b in zip(asked.value_function_approximator.weights, ctl.value_function_approximator.weights):
            a.copy_(b)
    assert torch.equal(asked.value_loss_gradient(xs, dones, costs), ctl.value_loss_gradient(xs, dones, costs))


def test_controller_falls_back_to_autograd_when_the_unit_is_refused():
    """The dense five-link manipulator: if the library refuses its train unit (a kernel would need scratch), the controller in automatic mode
    warns once with the library's message, trains through autograd and still rolls out on the fused kernels; fused_param_grad=True raises.
    If the unit is accepted, the controller fuses."""
    d = dyn("manip10")
    try:
        d.system.code_object(("train", "relu"))
        refused = False
    except NotImplementedError:
        refused = True
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        _, ctl = controller("manip10")
    mine = [w for w in seen if "fused parameter gradient" in str(w.message)]
    if not refused:
        assert ctl.fused_param_grad is True and not mine
        return
    assert len(mine) == 1 and "bytes of scratch" in str(mine[0].message)
    assert ctl.fused_param_grad is False and ctl.fused_value_grad
    with pytest.raises(NotImplementedError, match="bytes of scratch"):
        controller("manip10", fused_param_grad=True)
    xs, dones, costs = _batch(d, ctl, 64, 1)
    with pytest.raises(NotImplementedError, match="bytes of scratch"):
        _ops.value_loss_grad(d.system, ctl._task, ctl.value_function_approximator.descriptor(), xs, costs, dones)
    tot, h, t = ctl.params_update(xs, dones, costs, 0.1)               # autograd + the run-time compiled residual kernel
    assert all(np.isfinite(float(v)) for v in (tot, h, t))
