#!/usr/bin/env python3
"""Throughput of the fused rollout compiled at run time for a user-defined system (hjbx_system_enable_matrix_cores), next to
  (a) the built-in fused kernel of its twin (user planar quadrotor / Quadrotors2D, user cart-pole / Cartpole) -- the ceiling: the same
      arithmetic, compiled offline;
  (b) the path a user system has without matrix_cores: the PyTorch value network + one hjbx_vhjb_step_f32 launch per step.
The three are timed alternately in the same process: device events, --warmup untimed runs, median of --reps; B = 2^20 and 2^17
environments, T = 200 steps, forward Euler, float32, the benchmark's LQR-embedded ReLU network, an unbounded observation box so that every
environment stays live.  Also: the one-time compile cost of a matrix-core unit and of from_source itself (host clock around the call).
Prints one JSON line (profiles/user_fused.json keeps it next to the ISA table of tools/dev/user_fused_isa.py).

    python tools/dev/user_fused_bench.py [--steps 200] [--warmup 1] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from q_learning_with_hjb_amd import _abi, _ops  # noqa: E402
from q_learning_with_hjb_amd.configs import defaults as D  # noqa: E402
from q_learning_with_hjb_amd.controller.vhjb import VHJBController  # noqa: E402
from q_learning_with_hjb_amd.dynamics.cartpole import Cartpole  # noqa: E402
from q_learning_with_hjb_amd.dynamics.quadrotors import Quadrotors2D  # noqa: E402
from test_gpu_user_system import UserCartpole, UserQuad2D  # noqa: E402


class FusedQuad2D(UserQuad2D):
    def device_source(self):
        return dict(super().device_source(), matrix_cores=True)


class FusedCartpole(UserCartpole):
    def device_source(self):
        return dict(super().device_source(), matrix_cores=True)


def systems(name):
    """-> (user system with the matrix-core kernels, its built-in twin, the VHJB configuration)"""
    if name == "quad2d":
        cfg = D.quadrotors2d_dynamics_config()
        return FusedQuad2D(cfg), Quadrotors2D(cfg), D.quadrotors2d_vhjb_config()
    cfg = D.cartpole_dynamics_config()
    return FusedCartpole(cfg), Cartpole(cfg), D.cartpole_vhjb_config()


def timed(run, warmup, reps):
    for _ in range(warmup):
        run()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[1 << 20, 1 << 17])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("user_fused_bench: no HIP device (nothing is measured without one)")
    T = a.steps
    res, compile_s = {}, {}
    for name in ("quad2d", "cartpole"):
        t0 = time.perf_counter()
        du, db, vcfg = systems(name)
        t_create = time.perf_counter() - t0                     # (includes the built-in twin's handle: microseconds)
        ctl = VHJBController(du, vcfg, dtype=torch.float32, graph_updates=False)
        assert ctl.fused_value_grad
        vf = ctl.value_function_approximator
        vf.load_quadratic(ctl.P, noise=0.05, generator=torch.Generator(device="cuda").manual_seed(1234))
        desc = vf.descriptor()
        n, m = du.get_dimension()
        task = _abi.make_task(n, m, ctl.Q, ctl.R, ctl.P, ctl.xf, ctl.uf, None, None, ctl.epsilon, Rinv=ctl.R_inv)   # unbounded box
        t0 = time.perf_counter()
        du.system.code_object(("pd", "relu"))                   # the lazy compile, outside every timed window
        compile_s[name] = dict(from_source_s=round(t_create, 2), matrix_core_unit_s=round(time.perf_counter() - t0, 2))
        for B in a.batches:
            rng = np.random.default_rng(0)
            box = np.asarray(ctl.obs_max, np.float64).clip(max=3.0) * 0.2
            x0 = torch.as_tensor(np.asarray(ctl.xf, np.float64) + rng.uniform(-1, 1, (B, n)) * box, dtype=torch.float32, device="cuda").contiguous()
            ds = torch.full((B,), -1, dtype=torch.int32, device="cuda")
            last = {}

            def fused(system, key):
                def run():
                    ds.fill_(-1)
                    last[key] = _ops.vhjb_rollout(system, task, desc, x0, T, 1 << 30, ds, log_traj=False, want_x_out=True)["x_out"]
                return run

            xa, xb = torch.empty_like(x0), torch.empty_like(x0)
            cost, done = torch.empty((B,), device="cuda"), torch.empty((B,), device="cuda")

            def stepwise():
                ds.fill_(-1)
                xa.copy_(x0)
                cur, nxt = xa, xb
                with torch.no_grad():
                    for t in range(T):
                        g = vf.value_and_grad(cur)[1]
                        _ops.vhjb_step(du.system, task, t, 1 << 30, cur, g, nxt, cost, done, ds)
                        cur, nxt = nxt, cur
                last["stepwise"] = cur

            runs = dict(user_fused=fused(du.system, "user_fused"), builtin_fused=fused(db.system, "builtin_fused"), stepwise=stepwise)
            ts = {k: [] for k in runs}
            for k, fn in runs.items():                          # warm-up of every shape
                for _ in range(a.warmup):
                    fn()
            for _ in range(a.reps):                             # alternating
                for k, fn in runs.items():
                    ts[k] += timed(fn, 0, 1)
            torch.cuda.synchronize()
            row = {k: dict(env_steps_per_s=round(B * T / float(np.median(v)), 1), median_s=round(float(np.median(v)), 5),
                           min_s=round(min(v), 5), max_s=round(max(v), 5)) for k, v in ts.items()}
            row["live_fraction"] = float((ds < 0).double().mean().item())
            row["user_fused_equals_builtin_bitwise"] = bool(torch.equal(last["user_fused"], last["builtin_fused"]))
            row["user_over_builtin"] = round(row["user_fused"]["env_steps_per_s"] / row["builtin_fused"]["env_steps_per_s"], 4)
            row["user_fused_over_stepwise"] = round(row["user_fused"]["env_steps_per_s"] / row["stepwise"]["env_steps_per_s"], 3)
            res[f"{name}_B{B}"] = row
            del x0, xa, xb
        del ctl
    print(json.dumps(dict(tool="user_fused_bench", steps=T, warmup=a.warmup, reps=a.reps, integrator="euler", dtype="float32", activation="relu",
                          device=torch.cuda.get_device_name(0), compile=compile_s, cases=res)))


if __name__ == "__main__":
    main()
