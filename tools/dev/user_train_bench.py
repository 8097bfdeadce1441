#!/usr/bin/env python3
"""Time of the fused parameter gradient compiled at run time for a user-defined system (csrc/hjbx_user_train_kernels.hpp), next to
  (a) the built-in twin's k_train_coop (user planar quadrotor / Quadrotors2D, user cart-pole / Cartpole) -- the ceiling: the same
      template, compiled offline;
  (b) the path such a system had before: PyTorch autograd double back-prop + the run-time compiled residual kernel (the gradient of
      the two loss sums, what hjbx_value_loss_grad_f32 returns).
The three are timed alternately, case by case, in one process: device events, --warmup untimed calls, median and min-max of --reps; B = 256
(the reference's minibatch) and B = 2^20; float32, ReLU, normalised residual.  Separately: the fit phase's milliseconds per 256-sample
update under the captured fit graph (VHJBController.train, device-driven) for the user system fused, its built-in twin, and the user
system on autograd.  Also the one-time compile cost of the train unit (host clock).  Prints one JSON line (the `measured` block of
profiles/user_train.json).

    python tools/dev/user_train_bench.py [--warmup 3] [--reps 9] [--no-fit]
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

from q_learning_with_hjb_amd import _ops  # noqa: E402
from q_learning_with_hjb_amd.configs import defaults as D  # noqa: E402
from q_learning_with_hjb_amd.controller.vhjb import VHJBController  # noqa: E402
from q_learning_with_hjb_amd.dynamics.cartpole import Cartpole  # noqa: E402
from q_learning_with_hjb_amd.dynamics.quadrotors import Quadrotors2D  # noqa: E402
from test_gpu_user_system import UserCartpole, UserQuad2D  # noqa: E402


class FusedQuad2D(UserQuad2D):
    def device_source(self):
        return dict(super().device_source(), matrix_cores=True, param_grad=True)


class FusedCartpole(UserCartpole):
    def device_source(self):
        return dict(super().device_source(), matrix_cores=True, param_grad=True)


def systems(name):
    """-> (user system with the matrix-core kernels, its built-in twin, a function giving the VHJB configuration)"""
    if name == "quad2d":
        cfg = D.quadrotors2d_dynamics_config()
        return FusedQuad2D(cfg), Quadrotors2D(cfg), D.quadrotors2d_vhjb_config
    cfg = D.cartpole_dynamics_config()
    return FusedCartpole(cfg), Cartpole(cfg), D.cartpole_vhjb_config


def once(run):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    run()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return dict(median_ms=round(float(np.median(ms)), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4))


def fit_ms_per_update(dynamics, vcfg, **kw):
    """milliseconds of the fit phase per 256-sample update: train() of 3 epochs, the last epoch's fit phase on the host clock between two
    synchronisations, divided by its number of updates"""
    cfg = vcfg(epochs=3, num_of_trajectories_per_epoch=64, maximum_step=200, batch_size=256, maximum_buffer_size=1 << 16)
    ctl = VHJBController(dynamics, cfg, dtype=torch.float32, **kw)
    spans = []
    inner = ctl._fit_epoch_graphed if ctl._fit_graph_usable() else None
    if inner is not None:
        def timed(*a, **k):
            torch.cuda.synchronize()
            t0, c0 = time.perf_counter(), ctl.update_counter
            out = inner(*a, **k)
            torch.cuda.synchronize()
            spans.append((time.perf_counter() - t0, ctl.update_counter - c0))
            return out
        ctl._fit_epoch_graphed = timed
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ctl.train()
    torch.cuda.synchronize()
    total = time.perf_counter() - t0
    res = dict(fused_param_grad=bool(ctl.fused_param_grad), train_s=round(total, 3), updates=int(ctl.update_counter))
    if spans and spans[-1][1] > 0:
        res["fit_ms_per_update_last_epoch"] = round(1e3 * spans[-1][0] / spans[-1][1], 4)
    else:       # no device-driven fit phase (autograd path): the whole train() per update is the only clock there is
        res["train_ms_per_update"] = round(1e3 * total / max(1, ctl.update_counter), 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 1 << 20])
    ap.add_argument("--no-fit", action="store_true", help="skip the fit-phase timing")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("user_train_bench: no HIP device (nothing is measured without one)")
    cases, compile_s, fit = {}, {}, {}
    for name in ("quad2d", "cartpole"):
        du, db, vcfg = systems(name)
        t0 = time.perf_counter()
        du.system.code_object(("train", "relu"))                # the lazy compile, outside every timed window
        compile_s[name] = round(time.perf_counter() - t0, 2)
        ctl = VHJBController(du, vcfg(), dtype=torch.float32, graph_updates=False)
        slow = VHJBController(du, vcfg(), dtype=torch.float32, graph_updates=False, fused_param_grad=False)
        assert ctl.fused_param_grad and not slow.fused_param_grad
        vf = ctl.value_function_approximator
        vf.load_quadratic(ctl.P, noise=0.05, generator=torch.Generator(device="cuda").manual_seed(1234))
        with torch.no_grad():
            for w, v in zip(slow.value_function_approximator.weights, vf.weights):
                w.copy_(v)
        desc = vf.descriptor()
        n = du.state_dim
        for B in a.batches:
            rng = np.random.default_rng(0)
            box = np.asarray(ctl.obs_max, np.float64).clip(max=3.0) * 0.6
            xs = torch.as_tensor(np.asarray(ctl.xf, np.float64) + rng.uniform(-1, 1, (B, n)) * box, dtype=torch.float32, device="cuda").contiguous()
            dones = torch.as_tensor((rng.uniform(size=B) < 0.3).astype(np.float32), device="cuda")
            costs = torch.as_tensor(rng.uniform(0.5, 20, B).astype(np.float32), device="cuda")
            out_u, out_b = (torch.empty((2 * sum(p.numel() for p in vf.parameters()) + 4,), device="cuda") for _ in range(2))
            params = list(slow.value_function_approximator.parameters())

            def autograd():
                hs, _ = slow._hjb_sums(xs, dones)
                ts, _ = slow._termination_sums(xs, dones, costs)
                torch.autograd.grad(hs, params, retain_graph=True, allow_unused=True)
                torch.autograd.grad(ts, params, allow_unused=True)

            runs = dict(user_fused=lambda: _ops.value_loss_grad(du.system, ctl._task, desc, xs, costs, dones, out=out_u),
                        builtin_fused=lambda: _ops.value_loss_grad(db.system, ctl._task, desc, xs, costs, dones, out=out_b), autograd=autograd)
            if B > 1 << 17:
                del runs["autograd"]                            # (its activations for 2^20 samples x 2 graphs do not belong in a timing run)
            ts = {k: [] for k in runs}
            for fn in runs.values():
                for _ in range(a.warmup):
                    fn()
            for _ in range(a.reps):                             # alternating, case by case
                for k, fn in runs.items():
                    ts[k].append(once(fn))
            torch.cuda.synchronize()
            row = {k: stats(v) for k, v in ts.items()}
            rel = float((out_u.double() - out_b.double()).abs().max() / out_b.double().abs().max())
            row["user_vs_builtin_max_abs_over_max"] = rel
            row["user_over_builtin_median"] = round(row["user_fused"]["median_ms"] / row["builtin_fused"]["median_ms"], 4)
            row["user_within_builtin_min_max"] = bool(row["builtin_fused"]["min_ms"] <= row["user_fused"]["median_ms"] <= row["builtin_fused"]["max_ms"])
            if "autograd" in row:
                row["autograd_over_user_median"] = round(row["autograd"]["median_ms"] / row["user_fused"]["median_ms"], 2)
            cases[f"{name}_B{B}"] = row
        del ctl, slow
        if not a.no_fit:
            fit[name] = dict(user_fused=fit_ms_per_update(systems(name)[0], vcfg), builtin_fused=fit_ms_per_update(db, vcfg),
                             user_autograd=fit_ms_per_update(systems(name)[0], vcfg, fused_param_grad=False))
    print(json.dumps(dict(tool="user_train_bench", warmup=a.warmup, reps=a.reps, dtype="float32", activation="relu", residual="normalised",
                          device=torch.cuda.get_device_name(0), train_unit_compile_s=compile_s, cases=cases, fit_phase=fit)))


if __name__ == "__main__":
    main()
