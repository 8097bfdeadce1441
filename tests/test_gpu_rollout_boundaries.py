"""GPU tests of the seams of the fused value-gradient code (csrc/hjbx_mlp_core.hpp): where one product of mlp_value_grad ends and the next
begins, LDS operands are fetched ahead by inline asm and retired by counted waits -- the chains' rings and the grouped W1' rows of backward 1.
A read retired too early, a group walked in another order or a wait count off by one changes bits, so everything here is bitwise: the fused
rollout against step-by-step value_grad + vhjb_step launches at batch sizes around a tile (33 = one tile and one lane, so 31 padding lanes;
64; 97) and 1, 2 and 5 steps per launch, for both heads, the three activations and state dimensions 2 (layer-1 chain shorter than its
prefetch depth), 4, 6 and 10 (two, two and three float4s per W1' row); with env_order, with a tile that has nothing left to do (the arm that
skips the network), and value_grad without a gradient (the early return after V) between two full calls."""
import numpy as np
import pytest
import torch

from conftest import make_dynamics, make_vhjb_config
from q_learning_with_hjb_amd import _abi, _ops
from q_learning_with_hjb_amd.controller.vhjb import VHJBController

pytestmark = pytest.mark.gpu

T_MAX = 4            # the horizon ends at the fifth step: the longest launch below also runs the terminal step
STEPS = (1, 2, 5)
BATCHES = (33, 64, 97)
# (system, head, activation, integrator)
CONFIGS = [("cartpole", "pd", "relu", _abi.EULER), ("cartpole", "soft", "tanh", _abi.EULER), ("cartpole", "pd", "sin", _abi.EULER),
           ("quad2d", "pd", "tanh", _abi.EULER), ("quad2d", "soft", "relu", _abi.EULER),
           ("nearhover", "pd", "relu", _abi.RK4), ("nearhover", "soft", "tanh", _abi.RK4),
           ("linear", "pd", "sin", _abi.EULER), ("linear", "soft", "relu", _abi.EULER)]
STATE_DIM = {"linear": 2, "cartpole": 4, "quad2d": 6, "nearhover": 10}


def make(name, head, act, integ):
    d = make_dynamics(name)
    assert d.state_dim == STATE_DIM[name]
    d.integrator = integ
    kw = dict(value_structure="soft_pd") if head == "soft" else {}
    ctl = VHJBController(d, make_vhjb_config(name), dtype=torch.float32, activation=act, **kw)
    vf = ctl.value_function_approximator
    if head == "soft":                                      # non-zero biases on every layer
        gen = torch.Generator().manual_seed(4)
        with torch.no_grad():
            for p in vf.parameters():
                if p.dim() == 1:
                    p.copy_(0.1 * torch.randn(p.shape, generator=gen, dtype=torch.float64))
    rollout = _ops.softpd_rollout if head == "soft" else _ops.vhjb_rollout
    return d, ctl, vf, rollout


def start_states(d, ctl, B, seed):
    rng = np.random.default_rng(seed)
    box = np.asarray(ctl.obs_max, np.float64).clip(max=3.0)
    x = np.asarray(ctl.xf, np.float64) + rng.uniform(-1, 1, (B, d.state_dim)) * box * 1.03    # a few start outside the box: terminal at step 0
    return torch.as_tensor(x, dtype=torch.float32, device="cuda").contiguous()


def stepwise(d, ctl, vf, x0, ds0, n, integ):
    """n steps through hjbx_value_grad_f32 / hjbx_softpd_value_grad_f32 + hjbx_vhjb_step_f32; done_step after every step."""
    B = x0.shape[0]
    traj = torch.empty((n + 1, B, d.state_dim), device="cuda")
    cost = torch.empty((n, B), device="cuda")
    done = torch.empty_like(cost)
    ds, ds_after = ds0.clone(), []
    traj[0].copy_(x0)
    for t in range(n):
        g = vf.fused_value_grad(traj[t], want_v=False)[1]
        _ops.vhjb_step(d.system, ctl._task, t, T_MAX, traj[t], g, traj[t + 1], cost[t], done[t], ds, integrator=integ)
        ds_after.append(ds.clone())
    return traj, cost, done, ds_after


def assert_launch_equals(rollout, d, ctl, vf, x0, ds0, n, integ, ref, **kw):
    traj, cost, done, ds_after = ref
    ds = ds0.clone()
    one = rollout(d.system, ctl._task, vf.descriptor(), x0, n, T_MAX, ds, integrator=integ, **kw)
    assert torch.equal(one["traj"], traj[:n + 1]), "states"
    assert torch.equal(one["cost"], cost[:n]), "cost"
    assert torch.equal(one["done"], done[:n]), "done"
    assert torch.equal(ds, ds_after[n - 1]), "done_step"


@pytest.mark.parametrize("name,head,act,integ", CONFIGS, ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in CONFIGS])
def test_fused_rollout_bitwise_equals_stepwise_around_a_tile(name, head, act, integ):
    d, ctl, vf, rollout = make(name, head, act, integ)
    for B in BATCHES:
        x0 = start_states(d, ctl, B, 8 + B)
        ds0 = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        ref = stepwise(d, ctl, vf, x0, ds0, max(STEPS), integ)
        for n in STEPS:
            assert_launch_equals(rollout, d, ctl, vf, x0, ds0, n, integ, ref)
        assert int((ref[3][-1] >= 0).sum()) == B              # the horizon ended inside the longest launch


@pytest.mark.parametrize("name,head,act,integ", [CONFIGS[0], CONFIGS[6], CONFIGS[7]], ids=["cartpole-pd-relu", "nearhover-soft-tanh", "linear-pd-sin"])
def test_env_order_and_a_finished_tile(name, head, act, integ):
    """Tile 1 (environments 32..63) has finished before the launch and the kernel skips the network for it; its neighbours run it.  Then the
    same batch with a shuffled env_order, which mixes finished and live environments inside every tile."""
    d, ctl, vf, rollout = make(name, head, act, integ)
    B = 97
    x0 = start_states(d, ctl, B, 3)
    ds0 = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    ds0[32:64] = 0
    ds0[5] = 0
    ref = stepwise(d, ctl, vf, x0, ds0, max(STEPS), integ)
    assert float(ref[1][:, 32:64].abs().max()) == 0.0 and torch.equal(ref[0][-1, 32:64], x0[32:64])   # finished: zero cost, state held
    order = torch.randperm(B, generator=torch.Generator().manual_seed(1)).to(device="cuda", dtype=torch.int32)
    for n in STEPS:
        assert_launch_equals(rollout, d, ctl, vf, x0, ds0, n, integ, ref)
        assert_launch_equals(rollout, d, ctl, vf, x0, ds0, n, integ, ref, env_order=order)
    # every environment finished: no tile runs the network at all
    all_done = torch.zeros((B,), dtype=torch.int32, device="cuda")
    ref0 = stepwise(d, ctl, vf, x0, all_done, 2, integ)
    assert_launch_equals(rollout, d, ctl, vf, x0, all_done, 2, integ, ref0)
    assert float(ref0[1].abs().max()) == 0.0


@pytest.mark.parametrize("name,head,act,integ", [CONFIGS[0], CONFIGS[1], CONFIGS[5], CONFIGS[8]],
                         ids=["cartpole-pd-relu", "cartpole-soft-tanh", "nearhover-pd-relu", "linear-soft-relu"])
def test_value_without_gradient_between_full_calls(name, head, act, integ):
    """gout = NULL: the kernel returns after V.  Its waves then take their next tile group (2^18 states: several groups per wave), so
    whatever the early return leaves outstanding would meet the next tile's counted waits: V must be what the full call gives, and a full
    call afterwards must repeat the first one."""
    d, ctl, vf, _ = make(name, head, act, integ)
    for B in (33, 97, 1 << 18):
        x = start_states(d, ctl, B, 21)
        V, g = vf.fused_value_grad(x)
        V2, none = vf.fused_value_grad(x, want_grad=False)
        V3, g3 = vf.fused_value_grad(x)
        assert none is None and torch.equal(V2, V) and torch.equal(V3, V) and torch.equal(g3, g)
        assert bool(torch.isfinite(V).all()) and bool(torch.isfinite(g).all())
