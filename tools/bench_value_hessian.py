#!/usr/bin/env python3
"""Time of the value-network Hessian kernel (hjbx_value_hessian_f32) next to the torch closed form a user would otherwise run
(ValueFunctionApproximator.value_hessian in float32 on the same device).

Cart-pole (n = 4) and near-hover quadcopter (n = 10), B = 2^17 states, tanh and ReLU, H only.  The inputs rotate through --buffers state
buffers (no launch re-reads what the previous one left in the caches); after --warmup untimed rounds each timing is a device-event window
around --inner launches, and the figure is the median of --reps windows.  Written to profiles/value_hessian.json under "timing" (the parity
ratios of tests/test_gpu_value_hessian.py sit under "parity" in the same file) and printed as one JSON line:

  ms per launch, states/s, flop per state of the formulation (every chain a column runs, times the n columns of a state; the 32 - C n idle
  columns of a tile are NOT counted, so the fraction below is that of useful work), that over the 157.3 TFLOP/s float32 MFMA peak, and the
  speed-up over the torch form.

    python tools/bench_value_hessian.py [--batch 131072] [--reps 10] [--inner 20] [--warmup 2] [--buffers 4] [--head pd|soft_pd] [--user]

--head soft_pd times hjbx_softpd_value_hessian_f32 (the soft-PD network of the notebooks, biases seeded uniform(-0.5, 0.5)) next to
SoftPDValueFunctionApproximator.value_hessian in float32 for tanh and sin, and writes profiles/softpd_value_hessian.json instead; the
default, pd, is as described above.

--user times the kernel compiled at run time for a user-defined system (the user cart-pole and the user planar quadrotor of the tests, each
next to its built-in twin in alternating windows; an n = 8 system without a twin) and writes profiles/user_value_hessian.json: see main_user.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from q_learning_with_hjb_amd.configs import defaults as D  # noqa: E402
from q_learning_with_hjb_amd.controller.vhjb import VHJBController  # noqa: E402
from q_learning_with_hjb_amd.dynamics.cartpole import Cartpole  # noqa: E402
from q_learning_with_hjb_amd.dynamics.quadrotors import NearHoverQuadcopter  # noqa: E402

CASES = [("cartpole", "tanh"), ("cartpole", "relu"), ("nearhover", "tanh"), ("nearhover", "relu")]
SOFT_CASES = [("cartpole", "tanh"), ("cartpole", "sin"), ("nearhover", "tanh"), ("nearhover", "sin")]
PEAK_F32_MFMA = 157.3e12


def flop_per_state(n, activation):
    """What the kernel's formulation computes for one state: n columns, each its chains (2 flop per multiply-add) and the last product."""
    smooth = activation != "relu"
    layer1 = (4 if smooth else 3) * 2 * 128 * n                  # a1, a1. (again for act''), a1 again for the last product
    wide = (2 + (2 if smooth else 1)) * 2 * 128 * 128            # a2, a2.; r1. (and the sample's r1)
    narrow = 2 * (2 if smooth else 1) * 2 * 128 * 64             # y. (and y); r2. (and r2)
    return n * (layer1 + wide + narrow + 2 * 128 * n)


def make(name, activation, head="pd"):
    if name == "cartpole":
        d, cfg = Cartpole(D.cartpole_dynamics_config()), D.cartpole_vhjb_config()
    else:
        d, cfg = NearHoverQuadcopter(D.near_hover_dynamics_config()), D.near_hover_vhjb_config()
    ctl = VHJBController(d, cfg, activation=activation, graph_updates=False, value_structure=head)     # lecun-normal weights from the config's seed
    if head == "soft_pd":
        gen = torch.Generator().manual_seed(0)
        with torch.no_grad():
            for p in ctl.value_function_approximator.parameters():
                if p.dim() == 1:
                    p.copy_(torch.rand(p.shape, generator=gen) - 0.5)
    return d, ctl


def median_ms(fn, xs, warmup, reps, inner):
    k = 0
    for _ in range(warmup * len(xs)):
        fn(xs[k % len(xs)])
        k += 1
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            out = fn(xs[k % len(xs)])
            k += 1
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / inner)
        del out
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def main_user(args):
    """--user: the kernel compiled at run time for a user-defined system (hjbx_user_hessian_kernels.hpp) next to the built-in kernel of its
    twin -- user cart-pole / Cartpole, user planar quadrotor / Quadrotors2D: the same template, the same wrap, the same network and inputs --
    for tanh and sin, H only.  Per pair the two are timed in alternating windows of --inner launches (median of --reps windows each), then
    at B = 256: device time per launch and host time per call (the user kernel is launched by name through the module API, the twin through
    hipLaunchKernel).  Also: the host clock around the first call of each user unit (its compile), and an n = 8 system (four oscillators,
    two angles), which fills all 32 columns of a tile, with its fraction of the float32 MFMA peak.  Written under "timing" of
    profiles/user_value_hessian.json."""
    import time

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from q_learning_with_hjb_amd import _abi, _ops
    from q_learning_with_hjb_amd.dynamics.quadrotors import Quadrotors2D
    from test_user_fused_host import FusedCartpole, FusedQuad2D
    from test_user_hessian_host import n8_handle

    def pair(name):
        if name == "cartpole":
            cfg = D.cartpole_dynamics_config()
            return FusedCartpole(cfg), Cartpole(cfg), D.cartpole_vhjb_config()
        cfg = D.quadrotors2d_dynamics_config()
        return FusedQuad2D(cfg), Quadrotors2D(cfg), D.quadrotors2d_vhjb_config()

    def window(fn, xs, k, inner):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn(xs[k % len(xs)])
            k += 1
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / inner, k

    def alternate(fns, xs, inner):
        """-> per fn: [median, min, max] ms per launch over --reps windows, the fns taking turns"""
        k, times = 0, [[] for _ in fns]
        for _ in range(args.warmup):
            for f in fns:
                _, k = window(f, xs, k, len(xs))
        for _ in range(args.reps):
            for i, f in enumerate(fns):
                t, k = window(f, xs, k, inner)
                times[i].append(t)
        return [[round(float(np.median(t)), 5), round(float(np.min(t)), 5), round(float(np.max(t)), 5)] for t in times]

    def host_us_per_call(fn, x, calls=200):
        fn(x)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn(x)
        dt = time.perf_counter() - t0
        torch.cuda.synchronize()
        return round(dt / calls * 1e6, 2)

    res, compile_s = {}, {}
    for name in ("cartpole", "quad2d"):
        du, db, cfg = pair(name)
        n = du.state_dim
        for act in ("tanh", "sin"):
            ctl = VHJBController(db, cfg, activation=act, graph_updates=False)        # lecun-normal weights from the config's seed
            desc = ctl.value_function_approximator.descriptor()
            rng = np.random.default_rng(0)
            box = np.asarray(ctl.obs_max, np.float64).clip(max=3.0)
            xs = [torch.as_tensor(np.asarray(ctl.xf, np.float64) + rng.uniform(-1, 1, (args.batch, n)) * box, dtype=torch.float32, device="cuda").contiguous()
                  for _ in range(args.buffers)]
            user = lambda x: _ops.value_hessian(du.system, desc, x)[0]                # noqa: E731
            twin = lambda x: _ops.value_hessian(db.system, desc, x)[0]                # noqa: E731
            t0 = time.perf_counter()
            Hu = user(xs[0])
            torch.cuda.synchronize()
            compile_s[f"{name}_{act}"] = round(time.perf_counter() - t0, 2)
            equal = bool(torch.equal(Hu, twin(xs[0])))
            del Hu
            (u_ms, b_ms) = alternate([user, twin], xs, args.inner)
            small = [x[:256].contiguous() for x in xs]
            (u_small, b_small) = alternate([user, twin], small, 50)
            res[f"{name}_{act}"] = dict(n=n, user_ms=u_ms[0], user_ms_min_max=u_ms[1:], twin_ms=b_ms[0], twin_ms_min_max=b_ms[1:],
                                        user_over_twin=round(u_ms[0] / b_ms[0], 4), bit_equal=equal,
                                        b256=dict(user_us=round(u_small[0] * 1e3, 2), twin_us=round(b_small[0] * 1e3, 2),
                                                  user_host_us_per_call=host_us_per_call(user, small[0]), twin_host_us_per_call=host_us_per_call(twin, small[0])))
            del ctl, xs, small
            torch.cuda.empty_cache()
    # n = 8: no twin; its own lecun-normal network
    h8, n = n8_handle(), 8
    gen = torch.Generator().manual_seed(0)
    W = [(torch.randn((a, b), generator=gen).clamp(-2, 2) / 0.87962566103423978 / np.sqrt(a)).to("cuda").contiguous() for a, b in ((n, 128), (128, 128), (128, 64))]
    rng = np.random.default_rng(0)
    xs = [torch.as_tensor(rng.uniform(-3, 3, (args.batch, n)), dtype=torch.float32, device="cuda").contiguous() for _ in range(args.buffers)]
    for act in ("tanh", "sin", "relu"):
        desc = _abi.HjbxMlp()
        desc.W1, desc.W2, desc.W3 = (w.data_ptr() for w in W)
        desc.h1, desc.h2, desc.h3, desc.activation, desc.eps_scalar = 128, 128, 64, _abi._ACTIVATIONS[act], 0.01
        _abi._fill(desc.std, np.ones(n))
        fn = lambda x: _ops.value_hessian(h8, desc, x)[0]                             # noqa: E731
        t0 = time.perf_counter()
        fn(xs[0])
        torch.cuda.synchronize()
        compile_s[f"n8_{act}"] = round(time.perf_counter() - t0, 2)
        (ms,) = alternate([fn], xs, args.inner)
        flop = 8 * n * (128 * n + 128 * 128 + 128 * 64) * (0.7 if act == "relu" else 1.0)
        res[f"n8_{act}"] = dict(n=n, user_ms=ms[0], user_ms_min_max=ms[1:], states_per_s=round(args.batch / (ms[0] * 1e-3), 1), flop_per_state=flop,
                                fraction_of_f32_mfma_peak=round(flop * args.batch / (ms[0] * 1e-3) / PEAK_F32_MFMA, 4))
    timing = dict(tool="bench_value_hessian --user", B=args.batch, reps=args.reps, inner=args.inner, warmup=args.warmup, buffers=args.buffers,
                  device=torch.cuda.get_device_name(0), peak_f32_mfma_flops=PEAK_F32_MFMA, cases=res, first_call_seconds_including_compile=compile_s)
    out = args.out or os.path.join(ROOT, "profiles", "user_value_hessian.json")
    old = {}
    if os.path.exists(out):
        with open(out) as f:
            old = json.load(f)
    old["timing"] = timing
    with open(out, "w") as f:
        json.dump(old, f, indent=1, sort_keys=True)
    print(json.dumps(timing))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1 << 17)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--buffers", type=int, default=4)
    ap.add_argument("--head", choices=("pd", "soft_pd"), default="pd")
    ap.add_argument("--user", action="store_true", help="user-defined systems next to their built-in twins (profiles/user_value_hessian.json)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.user:
        if not torch.cuda.is_available():
            raise SystemExit("bench_value_hessian: needs an MI355X (there is no CPU path to time)")
        return main_user(args)
    soft = args.head == "soft_pd"
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "softpd_value_hessian.json" if soft else "value_hessian.json")
    if not torch.cuda.is_available():
        raise SystemExit("bench_value_hessian: needs an MI355X (there is no CPU path to time)")
    res = {}
    for name, act in (SOFT_CASES if soft else CASES):
        d, ctl = make(name, act, args.head)
        vf = ctl.value_function_approximator
        n = d.state_dim
        rng = np.random.default_rng(0)
        box = np.asarray(ctl.obs_max, np.float64).clip(max=3.0)
        xs = [torch.as_tensor(np.asarray(ctl.xf, np.float64) + rng.uniform(-1, 1, (args.batch, n)) * box, dtype=torch.float32, device="cuda").contiguous()
              for _ in range(args.buffers)]
        Hk, Ht = vf.fused_value_hessian(xs[0]), vf.value_hessian(xs[0])
        scale = Ht.abs().amax(dim=(1, 2), keepdim=True)
        agree = float(((Hk - Ht).abs() / scale).max().item())          # the two float32 evaluations timed here compute the same thing
        del Hk, Ht, scale
        k_ms, k_lo, k_hi = median_ms(vf.fused_value_hessian, xs, args.warmup, args.reps, args.inner)
        t_ms, t_lo, t_hi = median_ms(vf.value_hessian, xs, args.warmup, args.reps, max(1, args.inner // 10))
        # soft-PD: the formulation's own count, ten chains per column (the last product on the VALU is not counted)
        flop = 8 * n * (128 * n + 128 * 128 + 128 * 64) if soft else flop_per_state(n, act)
        res[f"{name}_{act}"] = dict(n=n, kernel_ms=round(k_ms, 4), kernel_ms_min_max=[round(k_lo, 4), round(k_hi, 4)],
                                    states_per_s=round(args.batch / (k_ms * 1e-3), 1), flop_per_state=flop,
                                    fraction_of_f32_mfma_peak=round(flop * args.batch / (k_ms * 1e-3) / PEAK_F32_MFMA, 4),
                                    torch_ms=round(t_ms, 4), torch_ms_min_max=[round(t_lo, 4), round(t_hi, 4)],
                                    speedup_over_torch=round(t_ms / k_ms, 2), max_kernel_vs_torch_rel=agree)
        del ctl, xs
        torch.cuda.empty_cache()
    timing = dict(tool="bench_value_hessian" + (" --head soft_pd" if soft else ""), B=args.batch, reps=args.reps, inner=args.inner, warmup=args.warmup, buffers=args.buffers,
                  device=torch.cuda.get_device_name(0), peak_f32_mfma_flops=PEAK_F32_MFMA, cases=res)
    old = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            old = json.load(f)
    old["timing"] = timing
    with open(args.out, "w") as f:
        json.dump(old, f, indent=1, sort_keys=True)
    print(json.dumps(timing))


if __name__ == "__main__":
    main()
