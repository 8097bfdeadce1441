"""Development aid: where one epoch of VHJBController.train goes -- rollout, the append of the rollout log to the replay ring, the fit phase,
and the wall time of the whole epoch -- for near-hover at B = 20, 2^17, 2^20 and cartpole at 2^20 (T = 200, ring of 10^6 records).

    python tools/dev/time_epoch.py [--torch-path] [--device-collection] [--only nearhover:131072] [--reps 5] [--out FILE] [--train-only]

Device events around each phase (the append includes its host read-back: the events see the idle device), medians over `--reps`
repetitions after one warm-up epoch, min and max beside them.  `--torch-path` appends with the masked transposed torch expression
written out below + ReplayBuffer.extend, and uses nothing newer than that: the same file runs on a tree from before
ReplayBuffer.extend_rollout existed, which is how the baseline is taken (both trees in one session, alternating).
`collect_wall_ms` is the host's share of data collection, on the host clock with the device synchronised at both ends: from before the start
states are drawn until x0 is resident on the device, plus the trajectory-cost statistics with their read-back.  `--device-collection`
constructs the controller with device_collection=True (sampler kernel + hjbx_rollout_cost_stats); without it these are the NumPy draw with
its three crossings and the masked (T+1, B) sum of train().  One JSON object."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--torch-path", action="store_true")
ap.add_argument("--device-collection", action="store_true", help="VHJBController(..., device_collection=True)")
ap.add_argument("--only", default=None, help="system:B, e.g. nearhover:131072")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
ap.add_argument("--label", default=None)
ap.add_argument("--train-only", action="store_true", help="only train(), one epoch at a time, `--reps` + 1 times: the run to put under "
                "`rocprofv3 --kernel-trace --stats` (kernel time per epoch = the trace's total / (reps + 1), against epoch_wall_ms)")
args = ap.parse_args()
if args.torch_path:
    os.environ["HJBX_DEVICE_APPEND"] = "0"       # (read by trees that have the device append: train() below then takes the torch path too)

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from q_learning_with_hjb_amd.configs import defaults as D
from q_learning_with_hjb_amd.controller.vhjb import VHJBController
from q_learning_with_hjb_amd.dynamics.cartpole import Cartpole
from q_learning_with_hjb_amd.dynamics.quadrotors import NearHoverQuadcopter

T, CAPACITY = 200, 10 ** 6
CTL_KW = dict(device_collection=True) if args.device_collection else {}      # (nothing passed without the flag: runs on older trees too)
CASES = [("nearhover", 20), ("nearhover", 1 << 17), ("nearhover", 1 << 20), ("cartpole", 1 << 20)]
if args.only:
    name, b = args.only.split(":")
    CASES = [(name, int(b))]


def make(name, B):
    kw = dict(epochs=1, num_of_trajectories_per_epoch=B, maximum_step=T, maximum_buffer_size=CAPACITY)
    if name == "nearhover":
        return VHJBController(NearHoverQuadcopter(D.near_hover_dynamics_config()), D.near_hover_vhjb_config(**kw), **CTL_KW)
    return VHJBController(Cartpole(D.cartpole_dynamics_config()), D.cartpole_vhjb_config(**kw), **CTL_KW)


def draw_x0(ctl, B):
    """the start states of an epoch as train() gets them"""
    if args.device_collection:
        return ctl._draw_start_states(B)
    return ctl._dev(ctl.dynamics.get_initial_state(batch_size=B))


def cost_statistics(ctl, out):
    """mean and standard deviation of the trajectory costs as train() gets them"""
    if args.device_collection:
        total, dev2, _, count = ctl._cost_stats(out)
        return total / count, (dev2 / count) ** 0.5
    ds = out["done_step"].long()
    valid = (torch.arange(T + 1, device=ctl.device)[:, None] <= ds[None, :])
    traj_costs = (out["cost"] * valid).sum(0).double().cpu().numpy()
    return float(traj_costs.sum() / len(traj_costs)), float(np.var(traj_costs) ** 0.5)


def stats(ms):
    return dict(median=float(np.median(ms)), min=float(min(ms)), max=float(max(ms)))


def event():
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def append_torch(ctl, out, valid, ds):
    """the append of train() before the device append existed"""
    vm = valid.t().reshape(-1)
    ctl.replay_buffer.extend(out["traj"].transpose(0, 1).reshape(-1, ctl.state_dim)[vm], out["cost"].t().reshape(-1)[vm], out["done"].t().reshape(-1)[vm])
    return int((ds + 1).sum().item())


def append_device(ctl, out, valid, ds):
    return ctl.replay_buffer.extend_rollout(out["traj"], out["cost"], out["done_step"])


def run_train_only(name, B):
    ctl = make(name, B)
    epoch_ms = []
    for rep in range(args.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctl.train()
        torch.cuda.synchronize()
        epoch_ms.append(1e3 * (time.perf_counter() - t0))
    return dict(system=name, B=B, T=T, capacity=CAPACITY, epochs=args.reps + 1, first_epoch_wall_ms=epoch_ms[0], epoch_wall_ms=stats(epoch_ms[1:]),
                all_epochs_wall_ms=float(sum(epoch_ms)))


def run_case(name, B):
    if args.train_only:
        return run_train_only(name, B)
    ctl = make(name, B)
    append = append_torch if args.torch_path else append_device
    rollout_ms, append_ms, append_wall_ms, fit_ms, epoch_ms, collect_ms, draw_ms, K = [], [], [], [], [], [], [], 0
    for rep in range(args.reps + 1):
        # the phases one by one
        torch.cuda.synchronize()
        d0 = time.perf_counter()
        x0 = draw_x0(ctl, B)
        torch.cuda.synchronize()
        d1 = time.perf_counter()
        e0 = event()
        out = ctl.rollout_batch(x0)
        e1 = event()
        torch.cuda.synchronize()
        s0 = time.perf_counter()
        cost_statistics(ctl, out)
        torch.cuda.synchronize()
        s1 = time.perf_counter()
        ds = out["done_step"].long()
        valid = (torch.arange(T + 1, device=ctl.device)[:, None] <= ds[None, :])
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        e2 = event()
        K = append(ctl, out, valid, ds)
        e3 = event()
        torch.cuda.synchronize()
        w1 = time.perf_counter()
        del out, valid, ds
        ctl.num_of_trajectories_per_epoch = 0                # an epoch without rollouts = the fit phase alone
        f0 = time.perf_counter()
        ctl.train()
        torch.cuda.synchronize()
        f1 = time.perf_counter()
        # ... and the epoch as train() runs it
        ctl.num_of_trajectories_per_epoch = B
        t0 = time.perf_counter()
        ctl.train()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if rep:
            rollout_ms.append(e0.elapsed_time(e1)); append_ms.append(e2.elapsed_time(e3)); append_wall_ms.append(1e3 * (w1 - w0))
            fit_ms.append(1e3 * (f1 - f0)); epoch_ms.append(1e3 * (t1 - t0))
            draw_ms.append(1e3 * (d1 - d0)); collect_ms.append(1e3 * (d1 - d0 + s1 - s0))
    n = ctl.state_dim
    landed = min(K, CAPACITY)
    # what the append has to move: the landed records read and written (x, cost; done written only) and done_step read twice
    moved = landed * (2 * (n + 1) + 1) * 4 + 2 * 4 * B
    src = torch.empty(max(1, moved // 8), dtype=torch.float32, device=ctl.device)
    dst = torch.empty_like(src)
    copy_ms = []
    for rep in range(args.reps + 3):
        c0 = event(); dst.copy_(src); c1 = event()
        torch.cuda.synchronize()
        if rep >= 3:
            copy_ms.append(c0.elapsed_time(c1))
    r = dict(system=name, B=B, T=T, capacity=CAPACITY, n=n, records_emitted=K, records_landed=landed, log_bytes=(T + 1) * B * (n + 1) * 4,
             rollout_ms=stats(rollout_ms), append_ms=stats(append_ms), append_wall_ms=stats(append_wall_ms), fit_wall_ms=stats(fit_ms),
             epoch_wall_ms=stats(epoch_ms), collect_wall_ms=stats(collect_ms), draw_wall_ms=stats(draw_ms), bytes_moved=moved, append_GBps=moved / (np.median(append_ms) * 1e-3) / 1e9,
             copy_same_bytes_ms=stats(copy_ms), updates_per_epoch=ctl.replay_buffer.num_batches(ctl.batch_size))
    rest = np.median(epoch_ms) - np.median(rollout_ms) - np.median(append_ms) - np.median(fit_ms)
    r["epoch_share_outside_rollout_append_fit"] = float(rest / np.median(epoch_ms))
    del ctl
    torch.cuda.empty_cache()
    return r


result = dict(tool="time_epoch", mode="torch-path" if args.torch_path else "device-append", device_collection=bool(args.device_collection), label=args.label, reps=args.reps,
              device=torch.cuda.get_device_name(0), cases=[run_case(name, B) for name, B in CASES])
line = json.dumps(result)
print(line, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
