"""Host-side checks of the fused value-gradient code's ISA (no GPU: hipcc cross-compiles for gfx950).  Every unit that includes
csrc/hjbx_mlp_core.hpp is compiled to assembly -- the five hjbx_mlp objects, the soft-PD rollout, both Hessians and the two parameter-gradient
units -- and every kernel of them must stay free of scratch and of spilled registers (a spill inside these kernels has produced wrong
trajectories before), inside the register budget its launch shape implies, and clean under tools/audit_asm_loads.py: no
compiler-generated instruction touches the destination of an inline-asm LDS read (the chains' operand rings, the grouped W1' rows of
backward 1) before the counted wait that retires it.  The cartpole ReLU f32 rollout kernel, the benchmark's, holds exactly the 784 MFMAs of
one tile-step: 776 of the five products and 8 of the layer-1 recomputation."""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "q_learning_with_hjb_amd", "csrc")
CORE_UNITS = ("hjbx_mlp.hip", "hjbx_softpd.hip", "hjbx_hessian.hip", "hjbx_softpd_hessian.hip", "hjbx_train.hip", "hjbx_train_coop.hip")
META = re.compile(r"\.max_flat_workgroup_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?"
                  r"\s+\.vgpr_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)")


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    """{object name: path of its device assembly}, compiled once, a few at a time"""
    from q_learning_with_hjb_amd import _abi
    out = tmp_path_factory.mktemp("isa")
    units = [(src, extra, obj) for src, extra, obj in _abi._UNITS if src in CORE_UNITS]
    assert len(units) == 15 and sum(u[0] == "hjbx_mlp.hip" for u in units) == 5

    def compile_one(u):
        src, extra, obj = u
        asm = str(out / obj.replace(".o", ".s"))
        r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=on", "-S", "--cuda-device-only"] + list(extra) +
                           ["-o", asm, os.path.join(CSRC, src)], stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        return obj, asm

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        return dict(ex.map(compile_one, units))


def test_no_scratch_no_spill_and_registers_within_the_launch_shape(isa):
    nkern = 0
    for obj, asm in isa.items():
        kernels = META.findall(open(asm).read())
        assert kernels, obj
        for wg, name, private, vgprs, spilled in kernels:
            nkern += 1
            assert int(spilled) == 0, f"{obj} {name}: {spilled} spilled VGPRs"
            # 512 threads = two waves per SIMD = 256 registers each; the one-wave-per-SIMD kernels (256 threads) have all 512
            assert int(vgprs) <= (256 if int(wg) > 256 else 512), f"{obj} {name}: {vgprs} VGPRs at {wg} threads per workgroup"
            # k_train_chains keeps small indexed stack objects by design (tests/test_host_logic.py); everything else has no scratch at all
            if "k_train_chains" not in name:
                assert int(private) == 0, f"{obj} {name}: {private} bytes of scratch"
    assert nkern >= 5 * 30 + 3 * 30


def test_inference_kernels_hold_256_registers_and_the_flagship_784_mfmas(isa):
    for obj in ("hjbx_mlp_relu.o", "hjbx_mlp_tanh.o", "hjbx_mlp_x3.o", "hjbx_mlp_h2.o", "hjbx_mlp_sin.o", "hjbx_softpd_relu.o", "hjbx_softpd_tanh.o",
                "hjbx_softpd_sin.o"):
        kernels = [k for k in META.findall(open(isa[obj]).read()) if "k_vhjb_rollout_mfma" in k[1] or "k_value_grad_mfma" in k[1]]
        assert len(kernels) == 30, (obj, len(kernels))
        for wg, name, private, vgprs, spilled in kernels:
            assert int(private) == 0 and int(spilled) == 0 and int(vgprs) <= 256, f"{obj} {name}: {private} B scratch, {spilled} spilled, {vgprs} VGPRs"
    # the benchmark's kernel: k_vhjb_rollout_mfma<EULER, Cartpole<float>, 8 waves, relu, f32, PD head>; its step loop is straight-line code
    text = open(isa["hjbx_mlp_relu.o"]).read()
    m = re.search(r"^_Z19k_vhjb_rollout_mfmaILi0EN4hjbx8CartpoleIfEELi8ELi0ELi0E9MlpHeadPdE\w*:[^\n]*\n(.*?)\n\s+s_endpgm", text, re.S | re.M)
    assert m, "flagship kernel not found"
    body = m.group(1)
    assert body.count("v_mfma_f32_32x32x2_f32") == 784
    # backward 1 fetches its 64 W1' rows by asm reads in groups (the compiler's own ds_read_b128 are the step's constants)
    assert len(re.findall(r";;#ASMSTART\n\s+ds_read_b128 ", body)) == 64


def test_asm_lds_reads_are_register_safe(isa):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import audit_asm_loads
    for obj, asm in isa.items():
        assert audit_asm_loads.audit(asm) == 0, obj
        assert audit_asm_loads.audit_mfma_asm_reads(asm) == 0, obj
