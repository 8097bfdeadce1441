#!/usr/bin/env python3
"""Time of the min-snap reference generator (hjbx_minsnap_reference_f32) and of the tracking rollout (hjbx_rollout_minsnap_tracking_f32)
next to the hover loop the library already had (hjbx_rollout_feedback_f32 of Quadrotors2D under its hover LQR) with the SAME logs: the same
log traffic without the planner's arithmetic.

Quadrotors2D, float32, Euler, T = 200 steps, one shared plan of S = 3 segments (the waypoints of the golden fixture at avg_speed 0.5: the
200 steps cross all three segments and end in the hover tail), B = 2^20 and 2^17 environments starting within +-0.3 of the first waypoint.
Every output buffer is allocated once; after --warmup untimed launches each timing is a device-event window around --inner launches of ONE
kernel, the windows of the kernels alternate, and the figure is the median of --reps windows.  Written to --out
(profiles/minsnap_tracking.json) and printed as one JSON line:

  ms per launch, algorithmic bytes per environment-step (what the launch must read and write, from the shapes, over B T), that traffic over
  the 8 TB/s HBM peak, and the tracking / hover ratio with full logs (traj, u, cost) and with no logs (x_final and total_cost only).

    python tools/bench_tracking.py [--batches 1048576 131072] [--steps 200] [--reps 7] [--inner 5] [--warmup 2] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from q_learning_with_hjb_amd import _abi, _ops  # noqa: E402
from q_learning_with_hjb_amd.configs import defaults as D  # noqa: E402
from q_learning_with_hjb_amd.controller.quadrotors_model_based_controller import (Quadrotors2DHoveringController,  # noqa: E402
                                                                                  Quadrotors2DTrackingController, Quadrotors2DWaypointsPlanner)
from q_learning_with_hjb_amd.dynamics.quadrotors import Quadrotors2D  # noqa: E402

PEAK_HBM = 8.0e12
W0 = [[0.0, 0.0], [1.0, 0.5], [1.5, -0.5], [0.0, 1.0]]
F = 4   # bytes per float32


def cases(quad, B, T):
    """name -> (launch function, algorithmic bytes of one launch)"""
    dev, f32 = torch.device("cuda"), torch.float32
    planner = Quadrotors2DWaypointsPlanner(np.array(W0), quad, avg_speed=0.5)
    assert planner.cumulated_t[-1] < T * quad.dt, "the horizon ends in the hover tail"
    track = Quadrotors2DTrackingController(quad, planner, np.eye(6), np.eye(2))
    hover = Quadrotors2DHoveringController(quad, np.zeros(6), np.eye(6), np.eye(2))
    coeff, cum_t, end_pt = planner.device_plan(f32, dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    x0 = ((torch.rand((B, 6), generator=gen, device=dev, dtype=f32) - 0.5) * 0.6).contiguous()
    traj = torch.empty((T + 1, B, 6), dtype=f32, device=dev)
    ulog = torch.empty((T, B, 2), dtype=f32, device=dev)
    cost = torch.empty((T + 1, B), dtype=f32, device=dev)          # (the hover loop logs T + 1 rows, the tracking loop T)
    x_ref = torch.empty((T, B, 6), dtype=f32, device=dev)
    u_ref = torch.empty((T, B, 2), dtype=f32, device=dev)
    total = torch.empty((B,), dtype=f32, device=dev)
    done_step = torch.empty((B,), dtype=torch.int32, device=dev)
    x_final = torch.empty((B, 6), dtype=f32, device=dev)
    L, sysp, st = _abi.lib(), quad.system.ptr, _ops._stream
    t_ctrl, t_task = track._descriptor(), track._task()
    h_ctrl = hover._descriptor()
    h_task = _abi.make_task(6, 2, np.eye(6), np.eye(2), hover.P, np.zeros(6), hover.uf, None, None, 0.0)
    p = _ops._p

    def reference():
        _abi.check(L.hjbx_minsnap_reference_f32(sysp, p(coeff), p(cum_t), p(end_pt), 3, 1, 0.0, T, p(x_ref), p(u_ref), B, st()))

    def tracking(logs, ref_logs=False):
        def run():
            _abi.check(L.hjbx_rollout_minsnap_tracking_f32(sysp, _abi.ref(t_task), _abi.ref(t_ctrl), _abi.EULER, p(coeff), p(cum_t), p(end_pt), 3, 1, 0.0, T,
                                                           p(x0), p(traj) if logs else None, p(ulog) if logs else None, p(cost) if logs else None, p(total),
                                                           p(x_final), p(x_ref) if ref_logs else None, p(u_ref) if ref_logs else None, B, st()))
        return run

    def hovering(logs):
        def run():
            _abi.check(L.hjbx_rollout_feedback_f32(sysp, _abi.ref(h_task), _abi.ref(h_ctrl), _abi.EULER, 0, T, p(x0), p(traj) if logs else None,
                                                   p(ulog) if logs else None, p(cost) if logs else None, p(done_step), p(total), p(x_final), B, st()))
        return run

    ends = B * (6 + 6 + 1) * F                 # x0 in, x_final and total_cost out
    return {
        "reference": (reference, B * T * (6 + 2) * F),
        "tracking_full_logs": (tracking(True), ends + B * ((T + 1) * 6 + T * 2 + T) * F),
        "hover_full_logs": (hovering(True), ends + B * F + B * ((T + 1) * 6 + T * 2 + (T + 1)) * F),
        "tracking_full_and_reference_logs": (tracking(True, True), ends + B * ((T + 1) * 6 + T * 2 + T + T * 8) * F),
        "tracking_no_logs": (tracking(False), ends),
        "hover_no_logs": (hovering(False), ends + B * F),
    }


def measure(fns, warmup, reps, inner):
    """median ms per launch of each function, the windows alternating between them"""
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
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1 << 20, 1 << 17])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "minsnap_tracking.json"))
    args = ap.parse_args()
    _ops.require_device()
    quad = Quadrotors2D(D.quadrotors2d_dynamics_config())
    T = args.steps
    result = dict(device=torch.cuda.get_device_name(0), system="Quadrotors2D", dtype="float32", integrator="euler", steps=T, segments=3,
                  reps=args.reps, inner=args.inner, warmup=args.warmup, peak_hbm_bytes_per_s=PEAK_HBM, batches={})
    for B in args.batches:
        cs = cases(quad, B, T)
        ms = measure({k: v[0] for k, v in cs.items()}, args.warmup, args.reps, args.inner)
        rows = {}
        for k, (_, nbytes) in cs.items():
            med, lo, hi = ms[k]
            rows[k] = dict(ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4), bytes_per_env_step=round(nbytes / (B * T), 3),
                           hbm_fraction=round(nbytes / (med * 1e-3) / PEAK_HBM, 4), env_steps_per_s=round(B * T / (med * 1e-3), 1))
        rows["tracking_over_hover_full_logs"] = round(ms["tracking_full_logs"][0] / ms["hover_full_logs"][0], 3)
        rows["tracking_over_hover_no_logs"] = round(ms["tracking_no_logs"][0] / ms["hover_no_logs"][0], 3)
        result["batches"][str(B)] = rows
        del cs
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
