#!/usr/bin/env python3
"""Host cost of a launch-bound streaming call: CALLS calls of hjbx_vhjb_step_f32 at B = 256 between two synchronisations, for the built-in
cart-pole and for the same cart-pole as a user-defined system (run-time compiled, launched by name).  The stepwise rollout makes T + 1 such
calls per rollout, so the host path of the entry point is what this times.  Prints one JSON object: microseconds per call, REPEATS times each.

    [HJBX_LIBRARY=<another build of libhjbx.so>] python tools/dev/time_stream_launch.py [--calls 1000] [--repeats 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from q_learning_with_hjb_amd import _abi, _ops  # noqa: E402

USER_CARTPOLE = r"""
    HJBX_DEV void wrap(T* x) const { x[1] = wrap_angle(x[1]); }
    HJBX_DEV void get_M(const T* x, T* Mq) const {
        T s, c; sincos_t(x[1], &s, &c);
        Mq[0] = p[0] + p[1]; Mq[1] = p[1] * p[2] * c; Mq[2] = p[1] * p[2] * c; Mq[3] = p[1] * p[2] * p[2];
    }
    HJBX_DEV void get_C(const T* x, T* Cq) const {
        T s, c; sincos_t(x[1], &s, &c);
        Cq[0] = T(0); Cq[1] = -p[1] * p[2] * x[3] * s; Cq[2] = T(0); Cq[3] = T(0);
    }
    HJBX_DEV void get_G(const T* x, T* Gq) const {
        T s, c; sincos_t(x[1], &s, &c);
        Gq[0] = T(0); Gq[1] = p[1] * p[3] * p[2] * s;
    }
    HJBX_DEV void get_B(T* Bq) const { Bq[0] = T(1); Bq[1] = T(0); }
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    B, params = 256, [1.0, 0.1, 0.5, 9.81]
    handles = {"builtin_cartpole": _abi.SystemHandle(_abi.SYS_CARTPOLE, 4, 1, 0.02, [-10.0], [10.0], params),
               "user_cartpole": _abi.SystemHandle.from_source(_abi.USER_MANIPULATOR, USER_CARTPOLE, 4, 1, 0.02, [-10.0], [10.0], params)}
    task = _abi.make_task(4, 1, np.eye(4), np.eye(1), np.eye(4), [0, np.pi, 0, 0], [0.0], [-5, -7, -10, -10], [5, 7, 10, 10], 1e-6)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    x = torch.rand((B, 4), generator=gen, device="cuda") - 0.5
    g = torch.rand((B, 4), generator=gen, device="cuda") - 0.5
    xn, c, d = torch.empty_like(x), torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
    ds = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    fn, st = _abi.lib().hjbx_vhjb_step_f32, torch.cuda.current_stream().cuda_stream
    out = dict(tool="tools/dev/time_stream_launch.py", library=os.path.basename(os.path.dirname(_abi._LIB_PATH)) + "/" + os.path.basename(_abi._LIB_PATH),
               entry_point="hjbx_vhjb_step_f32", B=B, calls=args.calls, us_per_call={})
    for name, h in handles.items():
        call = lambda: fn(h.ptr, _abi.ref(task), _abi.EULER, 0, 200, x.data_ptr(), g.data_ptr(), xn.data_ptr(), None, c.data_ptr(), d.data_ptr(),
                          ds.data_ptr(), None, B, st)
        for _ in range(200):                                                  # module load, clocks, caches
            _abi.check(call())
        runs = []
        for _ in range(args.repeats):
            ds.fill_(-1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.calls):
                call()
            torch.cuda.synchronize()
            runs.append(round((time.perf_counter() - t0) / args.calls * 1e6, 3))
        out["us_per_call"][name] = runs
    print(json.dumps(out))


if __name__ == "__main__":
    main()
