"""GPU tests of the matrix-core kernels compiled at run time for user-defined systems (hjbx_system_enable_matrix_cores): a `Dynamics`
subclass with matrix_cores=True in device_source() runs the value network and the whole closed loop in the two persistent MFMA kernels the
built-in systems use.

  * value gradient: the user planar quadrotor against the built-in Quadrotors2D kernel (same network code, same flags: bit for bit); a
    damped cart-pole -- a system without a built-in kernel -- against a float64 restatement, per element;
  * fused rollout == value_grad + vhjb_step applied step by step, bit for bit (three systems, PD and soft-PD head, Euler and RK4,
    horizon split with a shuffled env_order), with and without late workgroups;
  * against the oracle: the undamped user cart-pole is the oracle's cart-pole kind with the same constants -- T = 200 closed loop at 2^16
    environments judged by the oracle compiled for float (FACTOR = 2, as everywhere), `done_step` bit-equal outside the box / kink margins;
  * the controller: VHJBController takes the fused kernels for such a system (compaction, training, agreement with the unfused path).
"""
import numpy as np
import pytest
import torch

from conftest import make_vhjb_config, wrapped_diff
from netref import NetRef, smooth_term_scales
from oracle import oracle as O
from parity_util import F32_ULP, FACTOR, assert_within_cpu_yardstick, check, step_term_scales
from q_learning_with_hjb_amd import _abi, _ops
from q_learning_with_hjb_amd.configs import defaults as D
from q_learning_with_hjb_amd.controller.vhjb import VHJBController
from q_learning_with_hjb_amd.dynamics.quadrotors import Quadrotors2D
from test_gpu_user_system import CFG, UserCartpole
from test_user_fused_host import FusedCartpole, FusedQuad2D, Manip10

pytestmark = pytest.mark.gpu

RTOL = 1e-5      # the analytic per-element bound of test_gpu_f32_parity.py: |err| <= 1e-5 |want| + 1e-5 x (sum of the |terms| of that element)
DELTA = 1e-3     # margin to the observation box, in error-coordinate units (test_gpu_f32_parity.py)
KINK = 1e-5      # a ReLU unit is "at its kink" when |pre-activation| < KINK x (sum of |terms| of that unit) (test_gpu_f32_parity.py)
INTEG = {"euler": _abi.EULER, "rk4": _abi.RK4}


def make(name, activation="relu", soft=False, **kw):
    d = {"cartpole": lambda: FusedCartpole(D.cartpole_dynamics_config(**CFG)),
         "cartpole_damped": lambda: FusedCartpole(D.cartpole_dynamics_config(**CFG), damping=(0.4, 0.05)),
         "quad2d": lambda: FusedQuad2D(D.quadrotors2d_dynamics_config()),
         "manip10": lambda: Manip10(D.near_hover_dynamics_config())}[name]()
    cfg = make_vhjb_config({"cartpole": "cartpole", "cartpole_damped": "cartpole", "quad2d": "quad2d", "manip10": "nearhover"}[name])
    if soft:
        kw["value_structure"] = "soft_pd"
    return d, VHJBController(d, cfg, dtype=torch.float32, activation=activation, **kw)


def states(d, ctl, B, seed, frac):
    rng = np.random.default_rng(seed)
    box = np.asarray(ctl.obs_max, np.float64).clip(max=3.0) * frac
    x = np.asarray(ctl.xf, np.float64) + rng.uniform(-1, 1, (B, d.state_dim)) * box
    return torch.as_tensor(x, dtype=torch.float32, device="cuda").contiguous()


def randomize_biases(vf, seed, scale=0.1):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in vf.parameters():
            if p.dim() == 1:
                p.copy_(scale * torch.randn(p.shape, generator=gen, dtype=torch.float64))


def test_value_grad_of_the_user_quadrotor_is_the_builtin_kernels_bit_for_bit():
    """The user planar quadrotor (its wrap is the built-in one) with random weights, B = 3001 (ragged): V and dV/dx from the run-time
    compiled kernel against the built-in Quadrotors2D kernel on the same inputs.  The network code and the flags are the same."""
    du, ctl = make("quad2d")
    assert du.system.matrix_cores and ctl.fused_value_grad
    db = Quadrotors2D(D.quadrotors2d_dynamics_config())
    vf = ctl.value_function_approximator
    x = states(du, ctl, 3001, 4, 1.5)
    for act in ("relu", "tanh", "sin"):
        desc = vf.descriptor()
        desc.activation = _abi._ACTIVATIONS[act]
        Vu, gu = _ops.value_grad(du.system, desc, x)
        Vb, gb = _ops.value_grad(db.system, desc, x)
        assert torch.isfinite(Vb).all() and float(Vb.abs().max()) > 0
        assert torch.equal(Vu, Vb) and torch.equal(gu, gb), act
        V2, none = _ops.value_grad(du.system, desc, x, want_grad=False)
        assert none is None and torch.equal(V2, Vu)


def _net_f64(W, mean, std, eps, e, act):
    f, df = {"tanh": (np.tanh, lambda a: 1.0 - np.tanh(a) ** 2), "sin": (np.sin, np.cos)}[act]
    W1, W2, W3 = W
    z = (e - mean) / std
    a1 = z @ W1
    a2 = f(a1) @ W2
    y = f(a2) @ W3
    V = (y * y).sum(1) + eps * (e * e).sum(1)
    g = (((((2.0 * y) @ W3.T) * df(a2)) @ W2.T) * df(a1)) @ W1.T / std + 2.0 * eps * e
    return V, g


@pytest.mark.parametrize("act", ["relu", "tanh", "sin"])
def test_value_grad_of_a_system_without_a_builtin_kernel_vs_f64(act):
    """The damped cart-pole: V and dV/dx against the float64 restatement of tests/netref.py, per element at 1e-5 of the element's own term
    scale (ReLU: the environments with a unit within KINK of its kink are left out -- a float32 evaluation may take either side)."""
    d, ctl = make("cartpole_damped", act)
    vf = ctl.value_function_approximator
    B = 70001
    x = states(d, ctl, B, 2, 1.5)
    V, g = vf.fused_value_grad(x)
    W = [w.detach().cpu().numpy().astype(np.float64) for w in vf.weights]
    s = O.System(_abi.SYS_CARTPOLE, 4, 1, d.dt, d.umin, d.umax, [d.mc, d.mp, d.l, d.g])      # (the wrap of the user system is the cart-pole's)
    xr = x.cpu().numpy().astype(np.float64)
    mean, std, xf = (np.asarray(vf._np[k], np.float64)[None, :] for k in ("mean", "std", "xf"))
    if act == "relu":
        net = NetRef(W, vf._np["mean"], vf._np["std"], vf._np["xf"], vf.epsilon_scalar, lambda e: O.wrap(s, e))
        fw = net.forward(xr)
        oV, og = fw["V"], net.grad(fw)
        sV, sg, _ = net.term_scales(fw)
        c1, c2 = net.kink_candidates(fw, KINK)
        keep = ~(c1.any(1) | c2.any(1))
        assert keep.mean() > 0.97
    else:
        e = O.wrap(s, xr - xf)
        oV, og = _net_f64(W, mean, std, vf.epsilon_scalar, e, act)
        sV, sg = smooth_term_scales(W, mean, std, vf.epsilon_scalar, e, act)
        keep = np.ones(B, bool)
    rv = check(V.cpu().numpy()[keep], oV[keep], RTOL, sV[keep])
    rg = check(g.cpu().numpy()[keep], og[keep], RTOL, sg[keep])
    print(f"\ndamped cart-pole {act}: max err / (1e-5 |want| + 1e-5 term scale): V {rv:.3f}, gradV {rg:.3f}")


def _stepwise(d, ctl, x0, T, integ):
    vf = ctl.value_function_approximator
    B, n, m = x0.shape[0], d.state_dim, d.control_dim
    traj = torch.empty((T + 2, B, n), device="cuda")
    cost = torch.empty((T + 1, B), device="cuda")
    done, res = torch.empty_like(cost), torch.empty_like(cost)
    ul = torch.empty((T + 1, B, m), device="cuda")
    ds = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    traj[0].copy_(x0)
    for t in range(T + 1):
        g = vf.fused_value_grad(traj[t], want_v=False)[1]
        _ops.vhjb_step(d.system, ctl._task, t, T, traj[t], g, traj[t + 1], cost[t], done[t], ds, u_out=ul[t], integrator=integ, resid_t=res[t])
    return traj, cost, done, res, ul, ds


@pytest.mark.parametrize("integ", ["euler", "rk4"])
@pytest.mark.parametrize("name,act,soft", [("cartpole_damped", "tanh", False), ("quad2d", "relu", False), ("manip10", "sin", False),
                                           ("cartpole_damped", "tanh", True)])
def test_fused_rollout_bitwise_equals_stepwise(name, act, soft, integ):
    """hjbx_vhjb_rollout_f32 / hjbx_softpd_rollout_f32 on a user system == value_grad + hjbx_vhjb_step_f32 (the streaming kernel compiled at
    creation) applied T + 1 times, bit for bit, on every output; so does the horizon split 7 + 6 with a shuffled env_order."""
    d, ctl = make(name, act, soft)
    d.integrator = INTEG[integ]
    vf = ctl.value_function_approximator
    if soft:
        randomize_biases(vf, 4)
    elif act == "relu":   # the synthetic trained network of the built-in test: under random weights every quadrotor leaves the box within T steps
        vf.load_quadratic(ctl.P, noise=0.05, generator=torch.Generator(device="cuda").manual_seed(3))
    rollout = _ops.softpd_rollout if soft else _ops.vhjb_rollout
    B, T = 1000, 12                                           # ragged: 31 tiles + 8 environments
    x0 = states(d, ctl, B, 8, 1.03)                           # some start outside the box: terminal tuple at t = 0
    traj, cost, done, res, ul, ds = _stepwise(d, ctl, x0, T, INTEG[integ])
    ds1 = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    one = rollout(d.system, ctl._task, vf.descriptor(), x0, T + 1, T, ds1, integrator=INTEG[integ], log_u=True, log_residual=True, want_x_out=True)
    print(f"\n{name} {act} soft={soft} {integ}: {int((ds < T).sum())} of {B} environments end before T, {int((ds == 0).sum())} at t = 0")
    assert torch.isfinite(traj).all() and torch.isfinite(res).all()
    assert torch.equal(ds1, ds) and torch.equal(one["traj"], traj) and torch.equal(one["cost"], cost) and torch.equal(one["done"], done)
    assert torch.equal(one["u"], ul) and torch.equal(one["residual"], res) and torch.equal(one["x_out"], traj[T + 1])
    assert 0 < int((ds < T).sum()) < B
    ds2 = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    order = torch.randperm(B, generator=torch.Generator().manual_seed(1)).to(device="cuda", dtype=torch.int32)
    a = rollout(d.system, ctl._task, vf.descriptor(), x0, 7, T, ds2, integrator=INTEG[integ], log_traj=False, want_x_out=True)
    b = rollout(d.system, ctl._task, vf.descriptor(), a["x_out"], T + 1 - 7, T, ds2, t_first=7, integrator=INTEG[integ], env_order=order)
    assert torch.equal(ds2, ds) and torch.equal(b["traj"], traj[7:]) and torch.equal(torch.cat([a["cost"], b["cost"]]), cost)


def test_late_workgroups_do_not_change_results_and_the_workspace_is_left_zeroed():
    """The test hook for workgroups that cannot be resident before others finish (HJBX_OPT_ROLLOUT_EXTRA_WORKGROUPS) in the run-time
    compiled kernel: the same bits, with and without env_order, and the last wave's clean-up leaves the workspace all zero."""
    d, ctl = make("cartpole_damped", "tanh")
    vf = ctl.value_function_approximator
    B, K = 40000, 9
    x0 = states(d, ctl, B, 21, 1.02)
    order = torch.randperm(B, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)).to(torch.int32)
    ws = _ops._rollout_workspace(x0.device)

    def run(env_order=None):
        ds = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        out = _ops.vhjb_rollout(d.system, ctl._task, vf.descriptor(), x0, K, 1 << 30, ds, log_u=True, want_x_out=True, env_order=env_order)
        torch.cuda.synchronize()
        return out, ds
    try:
        ref, ds_ref = run()
        assert int(ws.abs().sum()) == 0 and 0 < int((ds_ref >= 0).sum()) < B
        for sched, extra, use_order in [(0, 1, False), (0, 3, True), (1, 0, False), (1, 2, True)]:
            _abi.set_option(_abi.OPT_ROLLOUT_SCHEDULE, sched)
            _abi.set_option(_abi.OPT_ROLLOUT_EXTRA_WORKGROUPS, extra)
            out, ds = run(order if use_order else None)
            tag = f"schedule {sched}, {extra} extra workgroups, order={use_order}"
            assert torch.equal(ds, ds_ref), tag
            for k in ("traj", "cost", "done", "u", "x_out"):
                assert torch.equal(out[k], ref[k]), (tag, k)
            assert int(ws.abs().sum()) == 0, tag + ": workspace not left zeroed"
    finally:
        _abi.set_option(_abi.OPT_ROLLOUT_SCHEDULE, 0)
        _abi.set_option(_abi.OPT_ROLLOUT_EXTRA_WORKGROUPS, 0)


def _oracle_side(d, ctl):
    vf = ctl.value_function_approximator
    s = O.System(_abi.SYS_CARTPOLE, 4, 1, d.dt, d.umin, d.umax, [d.mc, d.mp, d.l, d.g])
    W = [w.detach().cpu().numpy().astype(np.float64) for w in vf.weights]
    mlp = O.make_mlp(vf.features, vf._np["mean"], vf._np["std"], vf._np["xf"], vf.epsilon_scalar)
    return s, mlp, W


def _box_margins(s, ctl, traj):
    T1, B, n = traj.shape
    e = O.wrap(s, (traj.reshape(-1, n) - np.asarray(ctl.xf, np.float64)[None, :])).reshape(T1, B, n)
    omin, omax = np.asarray(ctl.obs_min, np.float64), np.asarray(ctl.obs_max, np.float64)
    return np.minimum(omax[None, None, :] - e, e - omin[None, None, :]).min(-1)


def test_closed_loop_T200_against_the_oracle():
    """The undamped user cart-pole with CFG's constants is the oracle's cart-pole kind with the same constants.  200 closed-loop steps
    under the LQR-embedded value network at B = 2^16, fused user kernel against the f64 oracle from the same float32 start states, next
    to the oracle compiled for float: median and p99 of the error at EVERY step within FACTOR x the CPU float32 loop's (floor 1e-3 of
    the 1e-5 bound), the median within the 1e-5 bound itself -- the assertions of test_closed_loop_error_curve_T200."""
    d, ctl = make("cartpole")
    assert ctl.fused_value_grad
    vf = ctl.value_function_approximator
    vf.load_quadratic(ctl.P, noise=0.05, generator=torch.Generator(device="cuda").manual_seed(1234))
    s, mlp, W = _oracle_side(d, ctl)
    B, T = 1 << 16, 200
    x0 = _ops.wrap(d.system, states(d, ctl, B, 13, 0.5))
    x0r = x0.cpu().numpy().astype(np.float64)
    ref = O.vhjb_rollout(s, ctl._task, mlp, *W, x0r, T)
    c32 = O.vhjb_rollout(s, ctl._task, mlp, *W, x0r, T, dtype=np.float32)
    rs = ref["done_step"]
    rng_k = np.abs(ref["traj"]).reshape(-1, 4).max(0)
    bound = RTOL * np.abs(ref["traj"]) + RTOL * np.maximum(rng_k, 1.0)[None, None, :]
    same_c = c32["done_step"] == rs
    ec = (np.abs(wrapped_diff(c32["traj"].astype(np.float64), ref["traj"], [1])) / bound).max(-1)
    out = ctl.rollout_batch(x0, max_steps=T)
    torch.cuda.synchronize()
    ds = out["done_step"].cpu().numpy()
    same = ds == rs
    err = np.abs(wrapped_diff(out["traj"].cpu().numpy().astype(np.float64), ref["traj"], [1]))
    eg = (err / bound).max(-1)
    both = same & same_c
    med_g, med_c = np.median(eg[:, both], axis=1), np.median(ec[:, both], axis=1)
    p99_g, p99_c = np.quantile(eg[:, both], 0.99, axis=1), np.quantile(ec[:, both], 0.99, axis=1)
    print(f"\nuser cart-pole T=200 B={B}: done_step agreement {same.mean():.5f} (CPU float32 {same_c.mean():.5f}), survive to T {np.mean(rs == T):.3f}; "
          f"worst step: median kernel / CPU {np.max(med_g[1:] / np.maximum(med_c[1:], 1e-3)):.2f}, p99 kernel / CPU "
          f"{np.max(p99_g[1:] / np.maximum(p99_c[1:], 1e-3)):.2f}, median / 1e-5 bound {med_g.max():.3f}")
    assert same.mean() > 0.999 and same.mean() >= same_c.mean() - 1e-3
    assert (med_g[1:] <= FACTOR * np.maximum(med_c[1:], 1e-3)).all()
    assert (p99_g[1:] <= FACTOR * np.maximum(p99_c[1:], 1e-3)).all()
    assert med_g.max() <= 1.0 and err.max() < 0.5


def test_done_step_bit_equal_to_the_oracle_outside_the_margins():
    """`done_step` of the fused user rollout == the f64 oracle's for every environment that, while alive, neither comes within DELTA of a
    face of the observation box nor passes a state with a ReLU unit within 10 KINK of its kink (the threshold the built-in test's
    explanation of a mismatch uses): 30 steps, B = 2^16, starts at 1.04x the box so that environments terminate throughout."""
    d, ctl = make("cartpole")
    vf = ctl.value_function_approximator
    vf.load_quadratic(ctl.P, noise=0.05, generator=torch.Generator(device="cuda").manual_seed(1234))
    s, mlp, W = _oracle_side(d, ctl)
    B, T = 1 << 16, 30
    rng = np.random.default_rng(12)
    box = np.asarray(ctl.obs_max, np.float64).clip(max=3.0) * 1.04
    box[2:] *= 0.3 / 1.04
    x0 = torch.as_tensor(np.asarray(ctl.xf, np.float64) + rng.uniform(-1, 1, (B, 4)) * box, dtype=torch.float32, device="cuda").contiguous()
    x0 = _ops.wrap(d.system, x0)
    ref = O.vhjb_rollout(s, ctl._task, mlp, *W, x0.cpu().numpy().astype(np.float64), T)
    rs = ref["done_step"]
    alive = np.arange(T + 1)[:, None] <= rs[None, :]
    near_box = ((np.abs(_box_margins(s, ctl, ref["traj"])) <= DELTA) & alive).any(0)
    assert 0.02 < (rs < T).mean() < 0.98 and near_box.mean() < 0.05
    out = ctl.rollout_batch(x0, max_steps=T)
    ds = out["done_step"].cpu().numpy()
    bad = np.nonzero(~near_box & (ds != rs))[0]
    net = NetRef(W, vf._np["mean"], vf._np["std"], vf._np["xf"], vf.epsilon_scalar, lambda e: O.wrap(s, e))
    unexplained = []
    for b in bad:
        last = int(min(ds[b], rs[b]))
        margin = net.kink_margin(net.forward(ref["traj"][: last + 1, b, :])).min()
        print(f"    done_step mismatch outside the box band: env {int(b)} got {int(ds[b])} want {int(rs[b])}, smallest kink margin on the way {margin:.2e}")
        if margin >= 10 * KINK:
            unexplained.append(int(b))
    print(f"\nuser cart-pole done_step: {near_box.mean():.3%} within {DELTA:g} of a box face, {(rs < T).mean():.1%} terminate before T, "
          f"{len(bad)} mismatches outside the band, {len(unexplained)} of them away from every kink")
    assert not unexplained


def test_controller_takes_the_fused_kernels_for_a_user_system():
    d, ctl = make("cartpole")
    assert ctl.fused_value_grad and not ctl.fused_param_grad
    plain = UserCartpole(D.cartpole_dynamics_config(**CFG))
    slow = VHJBController(plain, make_vhjb_config("cartpole"), dtype=torch.float32)
    assert not slow.fused_value_grad and not plain.system.matrix_cores
    with pytest.raises(NotImplementedError):
        _ops.value_grad(plain.system, slow.value_function_approximator.descriptor(), states(d, ctl, 64, 0, 0.5))
    # compaction: re-packing the live environments between chunks gives the single launch's bits
    vf = ctl.value_function_approximator
    vf.load_quadratic(ctl.P, noise=0.05, generator=torch.Generator(device="cuda").manual_seed(3))
    x0 = states(d, ctl, 20000, 9, 0.9)
    ctl.compaction_interval = 0
    full = ctl.rollout_batch(x0, max_steps=60)
    ctl.compaction_interval, ctl.compaction_min_batch = 16, 1
    chunked = ctl.rollout_batch(x0, max_steps=60)
    for k in ("traj", "cost", "done", "done_step"):
        assert torch.equal(full[k], chunked[k]), k
    assert int((full["done_step"] < 60).sum()) > 0
    # the unfused controller (PyTorch network + one vhjb_step launch per step: the path of a user system that did not ask) on the same
    # weights: the same done_step, and the first step's u and x' of BOTH within the float32 yardstick of the oracle (FACTOR = 2)
    unf = VHJBController(d, make_vhjb_config("cartpole"), dtype=torch.float32, fused_value_grad=False)
    assert not unf.fused_value_grad
    with torch.no_grad():
        for a, b in zip(unf.value_function_approximator.weights, vf.weights):
            a.copy_(b)
    B, T = 4096, 30
    x0 = _ops.wrap(d.system, states(d, ctl, B, 5, 0.5))
    of, ou_ = ctl.rollout_batch(x0, max_steps=T, log_u=True), unf.rollout_batch(x0, max_steps=T, log_u=True)
    assert torch.equal(of["done_step"], ou_["done_step"])
    s, mlp, W = _oracle_side(d, ctl)
    xr = x0.cpu().numpy().astype(np.float64)
    ds0 = np.full(B, -1, np.int32)
    _, g = O.value_grad(s, mlp, *W, xr)
    oxn, ou, oc, _, ods, _ = O.vhjb_step(s, ctl._task, 0, T, xr, g, ds0)
    _, g32 = O.value_grad(s, mlp, *W, xr, dtype=np.float32)
    cxn, cu, _, _, _, _ = O.vhjb_step(s, ctl._task, 0, T, xr, g32, ds0, dtype=np.float32)
    net = NetRef(W, vf._np["mean"], vf._np["std"], vf._np["xf"], vf.epsilon_scalar, lambda e: O.wrap(s, e))
    fw = net.forward(xr)
    _, gabs, _ = net.term_scales(fw)
    c1, c2 = net.kink_candidates(fw, KINK)
    keep = (ods < 0) & ~(c1.any(1) | c2.any(1))
    assert keep.mean() > 0.95
    S = step_term_scales("cartpole", d, ctl, s, xr, g, gabs, ou, oc)
    for label, o in (("fused", of), ("unfused", ou_)):
        assert_within_cpu_yardstick(f"{label} u[0]", o["u"][0], cu, ou, S["u"], keep=keep)
        assert_within_cpu_yardstick(f"{label} x[1]", o["traj"][1], cxn, oxn, S["x_next"], angle_idx=[1], keep=keep)
    # the learner: rollouts on the fused kernels, parameter gradient through autograd + the run-time compiled residual kernel
    ctl.epochs, ctl.num_of_trajectories_per_epoch = 2, 16
    lists = ctl.train()
    assert len(lists) == 6 and len(lists[0]) == 2 and all(np.isfinite(v) for lst in lists for v in lst)
