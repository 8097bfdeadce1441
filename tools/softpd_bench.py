#!/usr/bin/env python3
"""Throughput of the fused soft-PD closed loop (hjbx_softpd_rollout_f32) next to the PD kernel (hjbx_vhjb_rollout_f32) on the same run.

B = 2^20 environments, Euler, float32, features [128, 128, 64]: cartpole tanh and relu, near-hover quadcopter relu.  Both networks see the
same start states and a task whose observation box is unbounded, so every environment stays live for the whole launch and the two kernels
do the same amount of work per step (the soft-PD network: lecun-normal weights and small random biases; the PD network: the benchmark's
LQR-embedded weights with 5 % noise).  Each timing is one launch of --steps steps (after --warmup untimed launches), median of --reps.
Prints one JSON line: env-steps/s per case and network, and the soft-PD / PD ratio.

    python tools/softpd_bench.py [--steps 50] [--warmup 2] [--reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from q_learning_with_hjb_amd import _abi, _ops  # noqa: E402
from q_learning_with_hjb_amd.configs import defaults as D  # noqa: E402
from q_learning_with_hjb_amd.controller.vhjb import VHJBController  # noqa: E402
from q_learning_with_hjb_amd.dynamics.cartpole import Cartpole  # noqa: E402
from q_learning_with_hjb_amd.dynamics.quadrotors import NearHoverQuadcopter  # noqa: E402

CASES = [("cartpole", "tanh"), ("cartpole", "relu"), ("nearhover", "relu")]
B = 1 << 20


def make(name, act, structure):
    if name == "cartpole":
        d, cfg = Cartpole(D.cartpole_dynamics_config()), D.cartpole_vhjb_config()
    else:
        d, cfg = NearHoverQuadcopter(D.near_hover_dynamics_config()), D.near_hover_vhjb_config()
    d.integrator = _abi.EULER
    ctl = VHJBController(d, cfg, activation=act, value_structure=structure, graph_updates=False)
    vf = ctl.value_function_approximator
    if structure == "pd":
        vf.load_quadratic(ctl.P, noise=0.05, generator=torch.Generator(device="cuda").manual_seed(1234))
    else:
        gen = torch.Generator().manual_seed(1234)
        with torch.no_grad():
            for p in vf.parameters():
                if p.dim() == 1:
                    p.copy_(0.05 * torch.randn(p.shape, generator=gen))
    n, m = d.get_dimension()
    task = _abi.make_task(n, m, ctl.Q, ctl.R, ctl.P, ctl.xf, ctl.uf, None, None, ctl.epsilon, Rinv=ctl.R_inv)   # unbounded box
    return d, ctl, task


def time_rollout(fn, d, task, desc, x0, steps, warmup, reps):
    ds = torch.full((x0.shape[0],), -1, dtype=torch.int32, device="cuda")

    def run():
        ds.fill_(-1)
        return fn(d.system, task, desc, x0, steps, 1 << 30, ds, integrator=_abi.EULER, log_traj=False, want_x_out=True)

    for _ in range(warmup):
        run()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = run()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
    live = float((ds < 0).double().mean().item())
    finite = float(torch.isfinite(out["x_out"]).all(-1).double().mean().item())
    return x0.shape[0] * steps / float(np.median(times)), float(np.median(times)), live, finite


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    res = {}
    for name, act in CASES:
        row = {}
        for structure, fn in (("soft_pd", _ops.softpd_rollout), ("pd", _ops.vhjb_rollout)):
            d, ctl, task = make(name, act, structure)
            rng = np.random.default_rng(0)
            box = np.asarray(ctl.obs_max, np.float64).clip(max=3.0) * 0.2
            x0 = torch.as_tensor(np.asarray(ctl.xf, np.float64) + rng.uniform(-1, 1, (B, d.state_dim)) * box, dtype=torch.float32,
                                 device="cuda").contiguous()
            rate, sec, live, finite = time_rollout(fn, d, task, ctl.value_function_approximator.descriptor(), x0, args.steps, args.warmup,
                                                   args.reps)
            row[structure] = dict(env_steps_per_s=round(rate, 1), launch_ms=round(sec * 1e3, 3), live_fraction=live, finite_fraction=finite)
            del ctl
        row["soft_pd_over_pd"] = round(row["soft_pd"]["env_steps_per_s"] / row["pd"]["env_steps_per_s"], 4)
        res[f"{name}_{act}"] = row
    print(json.dumps(dict(tool="softpd_bench", B=B, steps=args.steps, warmup=args.warmup, reps=args.reps, integrator="euler", dtype="float32",
                          device=torch.cuda.get_device_name(0), cases=res,
                          min_soft_pd_over_pd=min(r["soft_pd_over_pd"] for r in res.values()))))


if __name__ == "__main__":
    main()
