#!/usr/bin/env python3
"""Time of the closed loop under a user-defined control law (hjbx_user_controller_rollout_f32: the law's snippet compiled at run time into
csrc/hjbx_user_controller_kernels.hpp) next to the built-in kernel for the same law (hjbx_rollout_feedback_f32 with the descriptor).

Two pairs, each the same arithmetic on both sides (the snippets of tests/user_laws.py restate controller_eval expression for expression
and the results are bit-equal, tests/test_gpu_user_controller.py): the cart-pole energy shaper (HJBX_CTRL_CARTPOLE_ENERGY) and the
Quadrotors2D hover LQR (HJBX_CTRL_LINEAR_FEEDBACK).  float32, Euler, B = 2^20 environments, T = 200 steps, traj + u + cost logs, a task
with the observation box off (every environment runs the whole horizon).  Every buffer is allocated once, and the two kernels of a pair
write the SAME buffers while they are timed (their outputs are compared bit for bit in separate buffers first): with a buffer set each,
where the buffers lay moved the ratio of one pair from 1.01 to 0.84 between two sessions.  After --warmup untimed launches
each timing is a device-event window around --inner launches of ONE kernel, the windows of the two kernels alternate, and the figures are
the median and the spread (min, max) of --reps windows.  The built-in kernel is the yardstick.  With the timings: VGPRs, spilled
registers and scratch bytes of the six run-time compiled kernels, read from the code object's metadata (llvm-readelf --notes).
Written to --out (profiles/user_controller.json) and printed as one JSON line.

    python tools/bench_user_controller.py [--batch 1048576] [--steps 200] [--reps 10] [--inner 3] [--warmup 2] [--out FILE]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import user_laws as UL  # noqa: E402
from q_learning_with_hjb_amd import _abi, _ops  # noqa: E402
from q_learning_with_hjb_amd.configs import defaults as D  # noqa: E402
from q_learning_with_hjb_amd.controller.cartpole_energy_shaping import CartpoleEnergyShapingController  # noqa: E402
from q_learning_with_hjb_amd.controller.quadrotors_model_based_controller import Quadrotors2DHoveringController  # noqa: E402
from q_learning_with_hjb_amd.dynamics.cartpole import Cartpole  # noqa: E402
from q_learning_with_hjb_amd.dynamics.quadrotors import Quadrotors2D  # noqa: E402

READELF = "/opt/rocm/llvm/bin/llvm-readelf"
META = re.compile(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.sgpr_count:\s+(\d+)\n(?:.*\n)*?\s+\.sgpr_spill_count:\s+(\d+)\n"
                  r"(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)")


def kernel_resources(code):
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(code)
        f.flush()
        notes = subprocess.run([READELF, "--notes", f.name], capture_output=True, text=True, check=True).stdout
    return {name: dict(scratch_bytes=int(priv), sgprs=int(sg), sgpr_spills=int(sgs), vgprs=int(vg), vgpr_spills=int(vgs))
            for name, priv, sg, sgs, vg, vgs in META.findall(notes)}


def pair(name, B, T):
    """-> ({"builtin": launch, "user_law": launch}, code object of the law, the two result dicts of one checked launch)"""
    dev, f32 = torch.device("cuda"), torch.float32
    if name == "cartpole_energy_shaping":
        d = Cartpole(D.cartpole_dynamics_config())
        c = CartpoleEnergyShapingController(d)
        x0 = np.array([0.0, 0.0, 0.0, 0.0]) + np.random.default_rng(0).uniform(-1, 1, (B, 4)) * [1.0, np.pi, 1.0, 1.0]
    else:
        d = Quadrotors2D(D.quadrotors2d_dynamics_config())
        c = Quadrotors2DHoveringController(d, np.zeros(6), np.eye(6), np.eye(2))
        x0 = np.random.default_rng(0).uniform(-0.8, 0.8, (B, 6))
    n, m = d.get_dimension()
    twin = UL.twin_of(c)
    x0 = torch.as_tensor(x0, dtype=f32, device=dev).contiguous()
    task = _abi.make_task(n, m, np.eye(n), np.eye(m), np.eye(n), c.xf, getattr(c, "uf", np.zeros(m)), None, None, 1e-10)
    bufs = [dict(traj=torch.empty((T + 1, B, n), dtype=f32, device=dev), u=torch.empty((T, B, m), dtype=f32, device=dev),
                 cost=torch.empty((T + 1, B), dtype=f32, device=dev), total=torch.empty((B,), dtype=f32, device=dev),
                 done=torch.empty((B,), dtype=torch.int32, device=dev), xf=torch.empty((B, n), dtype=f32, device=dev)) for _ in range(2)]
    L, p, st, desc, h = _abi.lib(), _ops._p, _ops._stream, c._descriptor(), twin.handle

    out = [0, 1]                         # which buffer set each kernel writes: separate for the comparison, THE SAME for the timing

    def builtin():
        o = bufs[out[0]]
        _abi.check(L.hjbx_rollout_feedback_f32(d.system.ptr, _abi.ref(task), _abi.ref(desc), _abi.EULER, 0, T, p(x0), p(o["traj"]), p(o["u"]), p(o["cost"]),
                                               p(o["done"]), p(o["total"]), p(o["xf"]), B, st()))

    def user_law():
        o = bufs[out[1]]
        _abi.check(L.hjbx_user_controller_rollout_f32(h.ptr, _abi.ref(task), _abi.EULER, 0, 0.0, T, p(x0), None, p(o["traj"]), p(o["u"]), p(o["cost"]),
                                                      p(o["done"]), p(o["total"]), p(o["xf"]), B, st()))

    builtin(); user_law()
    torch.cuda.synchronize()
    same = all(torch.equal(bufs[0][k].view(torch.int32), bufs[1][k].view(torch.int32)) for k in bufs[0])
    out[1] = 0                           # (where a buffer lies moves a streaming kernel's time by more than the two kernels differ)
    del bufs[1]
    torch.cuda.empty_cache()
    nbytes = B * (2 * n + 2) * 4 + B * ((T + 1) * n + T * m + (T + 1)) * 4
    return {"builtin": builtin, "user_law": user_law}, twin.code_object(), same, nbytes, (d, c, task, bufs)


def measure(fns, warmup, reps, inner):
    """ms per launch of each function in `reps` windows of `inner` launches, the windows alternating between the functions"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) / inner)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "user_controller.json"))
    args = ap.parse_args()
    _ops.require_device()
    B, T = args.batch, args.steps
    result = dict(device=torch.cuda.get_device_name(0), dtype="float32", integrator="euler", batch=B, steps=T, logs=["traj", "u", "cost"],
                  reps=args.reps, inner=args.inner, warmup=args.warmup, pairs={})
    for name in ("cartpole_energy_shaping", "quad2d_hover_lqr"):
        fns, code, same, nbytes, keep = pair(name, B, T)
        times = measure(fns, args.warmup, args.reps, args.inner)
        row = {}
        for k, v in times.items():
            med = float(np.median(v))
            row[k] = dict(ms_median=round(med, 4), ms_min=round(float(np.min(v)), 4), ms_max=round(float(np.max(v)), 4),
                          spread=round(float((np.max(v) - np.min(v)) / med), 4), algorithmic_bytes_per_s=round(nbytes / (med * 1e-3), 1))
        row["user_law_over_builtin"] = round(row["user_law"]["ms_median"] / row["builtin"]["ms_median"], 4)
        row["outputs_bit_equal"] = bool(same)
        row["kernels"] = kernel_resources(code)
        result["pairs"][name] = row
        del fns, keep
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
