"""ReplayBuffer.extend_rollout and hjbx_replay_append_* without a GPU: the ring semantics against the reference's deque(maxlen)
(controller/vhjb.py:62-73 extended trajectory by trajectory, :304-308), the argument validation of the C entry points (it returns
before anything touches the device) and the ISA audit of the new kernels."""
import os
import re
import subprocess
from collections import deque

import numpy as np
import pytest
import torch

from conftest import ROOT
from q_learning_with_hjb_amd import _abi
from q_learning_with_hjb_amd.controller.vhjb import ReplayBuffer


def _ring_in_order(rb):
    """logical (oldest -> newest) contents of the ring"""
    idx = torch.arange(rb.size) if rb.size < rb.capacity else (rb.head + torch.arange(rb.capacity)) % rb.capacity
    return rb.x[idx].numpy(), rb.cost[idx].numpy(), rb.done[idx].numpy()


def _log(rng, T, B, n, done_step):
    """a time-major log whose entries past done_step are NaN (nothing there may reach the ring)"""
    traj = rng.standard_normal((T + 1, B, n))
    cost = rng.standard_normal((T + 1, B))
    past = np.arange(T + 1)[:, None] > np.asarray(done_step)[None, :]
    traj[past] = np.nan
    cost[past] = np.nan
    return torch.from_numpy(traj), torch.from_numpy(cost), torch.as_tensor(done_step, dtype=torch.int32)


def _check_against_deque(capacity, n, appends, seed=0):
    """appends: list of (T, done_step list).  After each append the ring, read from `head`, equals the deque."""
    rng = np.random.default_rng(seed)
    rb = ReplayBuffer(n, capacity, torch.float64, "cpu")
    rb.x.fill_(float("nan")); rb.cost.fill_(float("nan")); rb.done.fill_(float("nan"))
    dq = deque(maxlen=capacity)
    head = 0
    for T, ds in appends:
        traj, cost, done_step = _log(rng, T, len(ds), n, ds)
        K = rb.extend_rollout(traj, cost, done_step)
        trajectories = []
        for b, d in enumerate(ds):
            trajectory = [(traj[t, b].numpy(), float(cost[t, b]), 1.0 if t == d else 0.0) for t in range(d + 1)]
            dq.extend(trajectory)                                                 # replay_buffer.xs.extend(trajectory), vhjb.py:308
            trajectories.append(trajectory)
        assert K == sum(len(t) for t in trajectories) == sum(d + 1 for d in ds)
        head = (head + min(K, capacity)) % capacity
        assert rb.head == head and rb.size == len(dq)
        x, c, dn = _ring_in_order(rb)
        assert len(x) == len(dq)
        if len(dq):
            assert np.array_equal(x, np.stack([r[0] for r in dq]))
            assert np.array_equal(c, np.array([r[1] for r in dq]))
            assert np.array_equal(dn, np.array([r[2] for r in dq]))
            assert not np.isnan(x).any() and not np.isnan(c).any()
    return rb


def test_extend_rollout_fewer_records_than_free_space():
    rb = _check_against_deque(50, 3, [(5, [2, 5, 0, 3])])
    assert rb.size == 14 and rb.head == 14 and torch.isnan(rb.x[14:]).all()     # no slot beyond the records was written


def test_extend_rollout_fills_the_ring_exactly():
    rb = _check_against_deque(14, 3, [(5, [2, 5, 0, 3])])
    assert rb.size == 14 and rb.head == 0


def test_extend_rollout_more_records_than_capacity():
    _check_against_deque(9, 2, [(5, [2, 5, 0, 3, 5, 5, 1])])


def test_extend_rollout_capacity_shorter_than_one_trajectory():
    _check_against_deque(4, 2, [(7, [7, 3, 7])])
    _check_against_deque(1, 2, [(7, [7, 3, 7])])


def test_extend_rollout_all_trajectories_of_one_record():
    _check_against_deque(10, 4, [(6, [0] * 7), (6, [0] * 7)])


def test_extend_rollout_several_appends_with_a_moving_head():
    rng = np.random.default_rng(3)
    appends = [(T, list(rng.integers(0, T + 1, size=B))) for T, B in ((6, 5), (3, 9), (10, 2), (6, 1), (4, 30), (6, 5), (2, 4))]
    rb = _check_against_deque(37, 3, appends, seed=4)
    assert rb.size == 37 and rb.head != 0


def test_extend_rollout_of_no_environment():
    rb = _check_against_deque(10, 3, [(4, [1, 2]), (4, []), (4, [4])])
    assert rb.size == 10 and rb.head == 0


def test_extend_rollout_rejects_done_steps_outside_the_log():
    rng = np.random.default_rng(1)
    for bad in (-1, 6):
        rb = ReplayBuffer(2, 10, torch.float64, "cpu")
        rb.x.fill_(7.0); rb.cost.fill_(7.0); rb.done.fill_(7.0)
        traj, cost, _ = _log(rng, 5, 3, 2, [1, 2, 3])
        with pytest.raises(ValueError, match="1 done_step entries outside"):
            rb.extend_rollout(traj, cost, torch.tensor([1, bad, 3], dtype=torch.int32))
        assert rb.head == 0 and rb.size == 0 and (rb.x == 7).all() and (rb.cost == 7).all() and (rb.done == 7).all()


# ---- the C entry points ------------------------------------------------------------------------------------------------------------------
def _call(sfx, **kw):
    """hjbx_replay_append_<sfx> with dummy (non-NULL, aligned, never dereferenced) pointers except where `kw` says otherwise"""
    a = dict(traj=0x1000, cost=0x2000, done_step=0x3000, T=5, B=3, n=4, buf_x=0x4000, buf_cost=0x5000, buf_done=0x6000, capacity=10, head=0,
             header=0x7000, workspace=0x8000, stream=None)
    a.update(kw)
    return getattr(_abi.lib(), f"hjbx_replay_append_{sfx}")(a["traj"], a["cost"], a["done_step"], a["T"], a["B"], a["n"], a["buf_x"], a["buf_cost"],
                                                            a["buf_done"], a["capacity"], a["head"], a["header"], a["workspace"], a["stream"])


def test_replay_append_symbols_are_exported():
    L = _abi.lib()
    for name in ("hjbx_replay_append_f32", "hjbx_replay_append_f64", "hjbx_replay_append_workspace_bytes"):
        assert hasattr(L, name) and name in _abi.EXPORTED_SYMBOLS
    # block sums / offsets only: a few bytes per 64 environments, and it grows with B
    small, big = L.hjbx_replay_append_workspace_bytes(1), L.hjbx_replay_append_workspace_bytes(1 << 20)
    assert 16 <= small <= 64 and small < big <= (1 << 20) // 64 * 12 + 64
    assert L.hjbx_replay_append_workspace_bytes(0) >= 8


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_replay_append_validates_before_any_launch(sfx):
    for name in ("traj", "cost", "done_step", "buf_x", "buf_cost", "buf_done", "header", "workspace"):
        assert _call(sfx, **{name: None}) == _abi.EINVAL, name
        assert "NULL" in _abi.last_error()
    for kw in (dict(n=0), dict(n=_abi.HJBX_MAX_N + 1), dict(n=-3), dict(B=-1), dict(T=-1), dict(capacity=0), dict(capacity=-5), dict(head=-1),
               dict(head=10), dict(head=11)):
        assert _call(sfx, **kw) == _abi.EINVAL, kw
        assert f"hjbx_replay_append_{sfx}" in _abi.last_error()
    with pytest.raises(ValueError):
        _abi.check(_call(sfx, head=10))
    assert _call(sfx, B=0) == _abi.OK


# ---- ISA audit ---------------------------------------------------------------------------------------------------------------------------
def test_replay_append_kernels_use_no_scratch(tmp_path):
    """Every instantiation of the three kernels: private segment 0, no spilled register (the zero-scratch audit of tests/test_host_logic.py)."""
    asm = tmp_path / "replay.s"
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=on", "-S", "--cuda-device-only", "-o", str(asm),
                    os.path.join(ROOT, "q_learning_with_hjb_amd", "csrc", "hjbx_replay.hip")], check=True, stderr=subprocess.DEVNULL)
    text = asm.read_text()
    meta = re.compile(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.sgpr_spill_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)")
    lds = re.compile(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n")
    kernels = meta.findall(text)
    copies = [k for k in kernels if "k_append_copy" in k[0]]
    # 16-byte words: records of 1..2 words with 4-byte costs (float32, n = 4, 8), 1..5 words with 8-byte costs (float64, even n);
    # 8-byte words: 1..5 words with 4-byte costs (float32, even n), 1..10 words with 8-byte costs (float64); 4-byte words: 1..10
    assert len(copies) == 2 + 5 + 5 + 10 + 10, len(copies)
    assert sum("k_append_slice_sums" in k[0] for k in kernels) == 1 and sum("k_append_scan" in k[0] for k in kernels) == 1
    assert len(kernels) == len(copies) + 2
    for name, private, sgpr_spill, vgpr_spill in kernels:
        assert int(private) == 0 and int(sgpr_spill) == 0 and int(vgpr_spill) == 0, f"{name}: {private} bytes of scratch, {sgpr_spill} + {vgpr_spill} spills"
    assert not re.search(r"^\s+scratch_(load|store)", text, flags=re.M) and "Folded Spill" not in text
    # the tile leaves room for at least two workgroups per CU (160 KiB of LDS): in fact three
    sizes = {name: int(size) for size, name in lds.findall(text)}
    assert len(sizes) == len(kernels)
    assert max(sizes.values()) <= 160 * 1024 // 3
    # the transposition is staged through LDS with 16- and 8-byte accesses on both sides where the record allows
    assert "ds_write_b64" in text and "ds_read_b64" in text and "global_load_dwordx2" in text and "global_store_dwordx2" in text
    assert "global_load_dwordx4" in text and "global_store_dwordx4" in text
