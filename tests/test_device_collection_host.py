"""Device-side data collection without a GPU: the NumPy restatement of Philox4x32-10 (tests/philox_ref.py, the yardstick of the sampler's
GPU tests) against the published Random123 known answers, the export and binding of the four new entry points, their argument validation
(it returns before anything touches the device) and the zero-scratch audit of the new kernels."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, make_dynamics
from philox_ref import philox4x32_10, uniforms
from q_learning_with_hjb_amd import _abi

NEW_SYMBOLS = ("hjbx_initial_state_philox_f32", "hjbx_initial_state_philox_f64", "hjbx_rollout_cost_stats_f32", "hjbx_rollout_cost_stats_f64")

# Random123 kat_vectors, philox4x32 with 10 rounds: (counter, key, output)
KNOWN_ANSWERS = [
    ("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


def _words(text):
    return np.array([int(w, 16) for w in text.split()], np.uint64)


@pytest.mark.parametrize("counter, key, output", KNOWN_ANSWERS)
def test_philox_restatement_reproduces_the_published_known_answers(counter, key, output):
    assert np.array_equal(philox4x32_10(_words(counter), _words(key)), _words(output).astype(np.uint32))


def test_philox_restatement_is_elementwise_over_batches():
    ctr = np.stack([_words(c) for c, _, _ in KNOWN_ANSWERS])
    key = np.stack([_words(k) for _, k, _ in KNOWN_ANSWERS])
    want = np.stack([_words(o) for _, _, o in KNOWN_ANSWERS]).astype(np.uint32)
    assert np.array_equal(philox4x32_10(ctr, key), want)


def test_reference_uniforms_follow_the_stream_definition():
    """word -> uniform as include/hjbx.h states it, on the all-zero known answer (seed 0, row 0, group 0), and the ranges."""
    w = [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    u32 = uniforms(0, 0, 1, 4, np.float32)[0]
    assert u32.dtype == np.float32 and [float(v) for v in u32] == [(x >> 8) / 2.0 ** 24 for x in w]
    u64 = uniforms(0, 0, 1, 2, np.float64)[0]
    assert [float(v) for v in u64] == [((w[0] >> 5) * 2 ** 26 + (w[1] >> 6)) / 2.0 ** 53, ((w[2] >> 5) * 2 ** 26 + (w[3] >> 6)) / 2.0 ** 53]
    for dtype in (np.float32, np.float64):
        u = uniforms(2 ** 64 - 1, 2 ** 32 - 3, 1000, 10, dtype)
        assert u.min() >= 0.0 and u.max() < 1.0 and 0.45 < u.mean() < 0.55
        # a row is a function of (seed, row) alone
        assert np.array_equal(u[5:9], uniforms(2 ** 64 - 1, 2 ** 32 - 3 + 5, 4, 10, dtype))


def test_new_symbols_are_exported_and_bound():
    L = _abi.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in _abi.EXPORTED_SYMBOLS
        assert getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == 8
    from q_learning_with_hjb_amd import _ops
    from q_learning_with_hjb_amd.dynamics.dynamics_basic import Dynamics
    assert callable(_ops.initial_state_philox) and callable(_ops.rollout_cost_stats) and callable(Dynamics.sample_initial_states)
    with open(os.path.join(ROOT, "include", "hjbx.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\bint {name}\(", header), name


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_initial_state_philox_validates_before_any_launch(sfx):
    d = make_dynamics("cartpole")                         # (creating a built-in handle needs no device)
    mean, std = np.zeros(4), np.ones(4)
    fn = getattr(_abi.lib(), f"hjbx_initial_state_philox_{sfx}")

    def call(sys=d.system.ptr, mean=mean.ctypes.data, std=std.ctypes.data, x0=0x1000, B=3):
        return fn(sys, mean, std, 7, 0, x0, B, None)

    for kw in (dict(sys=None), dict(mean=None), dict(std=None), dict(x0=None), dict(B=-1), dict(x0=0x1004)):
        assert call(**kw) == _abi.EINVAL, kw
        assert _abi.last_error()
    assert call(B=0) == _abi.OK


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_rollout_cost_stats_validates_before_any_launch(sfx):
    fn = getattr(_abi.lib(), f"hjbx_rollout_cost_stats_{sfx}")

    def call(cost=0x1000, done_step=0x2000, S=5, B=3, traj_cost=0x3000, stats=0x4000, workspace=0x5000):
        return fn(cost, done_step, S, B, traj_cost, stats, workspace, None)

    for name in ("cost", "done_step", "stats", "workspace"):
        assert call(**{name: None}) == _abi.EINVAL, name
        assert "NULL" in _abi.last_error()
    for kw in (dict(B=-1), dict(S=0), dict(S=-2), dict(stats=0x4004), dict(traj_cost=0x3004), dict(workspace=0x5008), dict(done_step=0x2002)):
        assert call(**kw) == _abi.EINVAL, kw
        assert f"hjbx_rollout_cost_stats_{sfx}" in _abi.last_error()
    assert call(B=0) == _abi.OK
    assert call(B=0, traj_cost=None) == _abi.OK


def test_python_wrappers_check_their_arguments():
    import torch
    from q_learning_with_hjb_amd import _ops
    d = make_dynamics("cartpole")
    for kw in (dict(batch_size=-1, seed=0), dict(batch_size=1, seed=-1), dict(batch_size=1, seed=1 << 64), dict(batch_size=1, seed=0, first_row=1 << 64),
               dict(batch_size=2, seed=0, first_row=(1 << 64) - 1)):
        with pytest.raises(ValueError):
            _ops.initial_state_philox(d.system, d.x0_mean, d.x0_std, device="cpu", **kw)
    with pytest.raises(TypeError):                         # not a device tensor
        _ops.rollout_cost_stats(torch.zeros(3, 2), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError):
        _ops.rollout_cost_stats(torch.zeros(3), torch.zeros(3, dtype=torch.int32))


def test_new_kernels_use_no_scratch(tmp_path):
    """The two statistics kernels (float32 / float64 logs), the fused sampler kernels (every built-in system x two precisions) and the
    two uniform-fill kernels of the user-system path: private segment 0, no spilled register; the Philox rounds stay in registers as plain
    32 x 32 -> 64 multiplies; the sampler reads no global memory at all and nothing here uses an atomic on floating-point data."""
    csrc = os.path.join(ROOT, "q_learning_with_hjb_amd", "csrc")
    procs = []
    for unit in ("hjbx_collect", "hjbx_kernels"):
        procs.append(subprocess.Popen(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=on", "-S", "--cuda-device-only",
                                       "-o", str(tmp_path / f"{unit}.s"), os.path.join(csrc, f"{unit}.hip")], stderr=subprocess.DEVNULL))
    assert all(p.wait() == 0 for p in procs)
    meta = re.compile(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.sgpr_spill_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)")
    collect = (tmp_path / "hjbx_collect.s").read_text()
    kernels = meta.findall(collect)
    assert len(kernels) == 4 and sum("k_cost_sums" in k[0] for k in kernels) == 2 and sum("k_cost_spread" in k[0] for k in kernels) == 2, kernels
    assert not re.search(r"^\s+scratch_(load|store)", collect, flags=re.M) and "Folded Spill" not in collect
    assert not re.search(r"atomic_(add|pk_add|fadd)_f", collect)
    streaming = meta.findall((tmp_path / "hjbx_kernels.s").read_text())
    new = [k for k in streaming if "k_initial_state_philox" in k[0] or "k_philox_uniforms" in k[0]]
    # one fused sampler kernel per instantiation of k_initial_state (the built-in systems, every dimension of the linear one, x two precisions)
    assert sum("k_initial_state_philox" in k[0] for k in new) == sum("k_initial_stateI" in k[0] for k in streaming) >= 10, [k[0] for k in new]
    assert sum("k_philox_uniforms" in k[0] for k in new) == 2
    for name, private, sgpr_spill, vgpr_spill in kernels + new:
        assert int(private) == 0 and int(sgpr_spill) == 0 and int(vgpr_spill) == 0, f"{name}: {private} bytes of scratch, {sgpr_spill} + {vgpr_spill} spills"
    # the body of one fused sampler kernel: multiplies of the rounds, row stores, and not a single load from global memory
    text = (tmp_path / "hjbx_kernels.s").read_text()
    for name in (k[0] for k in new if "k_initial_state_philox" in k[0]):
        body = text.split(f"\n{name}:", 1)[1].split("s_endpgm", 1)[0]
        assert ("v_mul_hi_u32" in body or "v_mad_u64_u32" in body) and "global_store" in body, name
        assert "global_load" not in body and "flat_load" not in body and "atomic" not in body, name
