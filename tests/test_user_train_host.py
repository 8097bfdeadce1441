"""CPU-only tests of the fused parameter gradient for user-defined systems (csrc/hjbx_user_train_kernels.hpp): a `Dynamics` subclass whose
device_source() says matrix_cores=True gets the cooperative kernel k_train_coop -- the template the built-in systems run, hoisted into
csrc/hjbx_train_coop_kernels.hpp -- compiled for its own struct at first use, one unit of four kernels (residual mode 0 / 1 x PS 1 / 4) per
activation.  Here, without a device: the lazy compile and what the LOADED code objects hold (kernels, scratch, registers, argument layout),
the refusal of a whole unit when one kernel needs scratch (the dense five-link manipulator) and what the controller makes of it, the ISA
audits of the unit, the entry points' refusals, a compile failure only this unit has, the header, and the recorded equality of the
built-in instruction streams before and after the hoist.  No compute call touches a GPU."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import time
import warnings

import pytest
import torch

from conftest import ROOT, make_vhjb_config
from q_learning_with_hjb_amd import _abi
from q_learning_with_hjb_amd.configs import defaults as D
from q_learning_with_hjb_amd.controller.vhjb import VHJBController
from test_gpu_user_system import CARTPOLE_SRC, CFG, QUAD2D_SRC, UserQuad2D
from test_user_fused_host import (CSRC, HIPCC, MANIP10_SRC, META, OBJDUMP, READELF, FusedCartpole, FusedQuad2D, Manip10, _fake_mlp,
                                  fused_systems, kernel_metadata)

ACTS = ("relu", "tanh", "sin")


def _asking(cls):
    """`cls` (a Dynamics subclass with matrix_cores=True) also asking for the fused parameter gradient: param_grad=True in device_source()"""
    return type("Train" + cls.__name__, (cls,), {"device_source": lambda self: dict(cls.device_source(self), param_grad=True)})


def train_systems():
    """fused_systems() of tests/test_user_fused_host.py, each asking VHJBController for the fused parameter gradient as well"""
    return {"cartpole_damped": lambda: _asking(FusedCartpole)(D.cartpole_dynamics_config(**CFG), damping=(0.4, 0.05)),
            "quad2d": lambda: _asking(FusedQuad2D)(D.quadrotors2d_dynamics_config()),
            "manip10": lambda: _asking(Manip10)(D.near_hover_dynamics_config())}
KERNEL = re.compile(r"_Z12k_train_coopILi(\d)ELi(\d)ELi(\d)EN4hjbx10UserSystemIfEEE")


def _loaded_unit_is_clean(h, act, tmp_path, tag):
    """the four kernels of the train unit the handle really loads: names, zero scratch, zero spilled VGPRs, <= 512 VGPRs"""
    code = h.code_object(("train", act))
    assert h.code_object(("train", act)) == code                                              # the same object on every request
    path, kernels = kernel_metadata(code, tmp_path, tag)
    found = sorted(tuple(int(v) for v in KERNEL.match(k[0]).groups()) for k in kernels if KERNEL.match(k[0]))
    a = _abi._ACTIVATIONS[act]
    assert len(kernels) == 4 and found == [(0, a, 1), (0, a, 4), (1, a, 1), (1, a, 4)], [k[0] for k in kernels]
    for kname, private, sgpr_spill, vgprs, vgpr_spill in kernels:
        print(f"    {tag} {kname[:30]}: {vgprs} VGPRs, {vgpr_spill} spilled VGPRs, {sgpr_spill} spilled SGPRs, {private} bytes of scratch")
        assert int(private) == 0 and int(vgpr_spill) == 0, f"{kname}: {private} bytes of scratch, {vgpr_spill} spilled VGPRs"
        assert int(vgprs) <= 512, f"{kname}: {vgprs} VGPRs do not fit one wave per SIMD"
    dis = subprocess.run([OBJDUMP, "-d", str(path)], capture_output=True, text=True, check=True).stdout
    assert dis.count("v_mfma_f32_32x32x2_f32") >= 2 * 600 + 2 * 400       # a tile's chains and outer products, PS 1 and PS 4 (n = 4: 692 and 500)
    return path, code


@pytest.mark.parametrize("name", ["cartpole_damped", "quad2d"])
def test_train_unit_compiles_lazily_and_the_loaded_kernels_have_no_scratch(name, tmp_path):
    """Damped cart-pole (n = 4) and user planar quadrotor (n = 6): creating and enabling the handle compiles nothing new; the first request
    for an activation compiles that unit, once; all four kernels of the loaded code object are free of scratch and of spilled VGPRs.  sin
    exists for n <= 4, as built in.  A second handle of the same system gets the same code object without another compile."""
    t0 = time.perf_counter()
    d = fused_systems()[name]()
    t_create = time.perf_counter() - t0
    h = d.system
    assert h.kind == _abi.SYS_USER and h.matrix_cores
    times = {}
    for act in ACTS:
        if act == "sin" and h.n > 4:
            t0 = time.perf_counter()
            with pytest.raises(NotImplementedError, match="n <= 4"):
                h.code_object(("train", act))
            assert time.perf_counter() - t0 < 0.5
            continue
        t0 = time.perf_counter()
        h.code_object(("train", act))
        times[act] = time.perf_counter() - t0
        _, code = _loaded_unit_is_clean(h, act, tmp_path, f"{name}_{act}")
        # lazy, and once per handle: this handle's first request took a compile, its second one is a copy (compared with each other, not with
        # a wall-clock threshold: hiprtc needs seconds for the four kernels on any machine, the copy microseconds)
        t0 = time.perf_counter()
        assert h.code_object(("train", act)) == code
        assert time.perf_counter() - t0 < times[act] / 10, (act, times)
    print(f"\n{name}: from_source {t_create:.1f} s; train units " + ", ".join(f"{a} {t:.1f} s" for a, t in times.items()))


def test_kernel_argument_layout_matches_the_host_structs(tmp_path):
    """The by-value arguments the host builds (hjbx_train_coop.hip: system blob, MlpP<N>, TaskP<float, N, M>, Limits<float, M>) against the
    argument sizes in the loaded code object's metadata, user quadrotor (n = 6, m = 2, four parameters)."""
    h = fused_systems()["quad2d"]().system
    path = tmp_path / "quad2d_train.co"
    path.write_bytes(h.code_object(("train", "relu")))
    notes = subprocess.run([READELF, "--notes", str(path)], capture_output=True, text=True, check=True).stdout
    n, m, npar = 6, 2, 4
    want = [4 * npar, 4 * (3 * n + 1), 4 * (2 * n * n + 2 * m * m + 3 * n + m + 3), 4 * (2 * m + 1)] + [8] * 6 + [4] + [8] * 5
    blocks = notes.split(".args:")[1:]
    assert len(blocks) == 4
    for blk in blocks:
        blk = blk.split(".group_segment_fixed_size")[0]
        sizes = [int(s) for s, kind in re.findall(r"\.size:\s+(\d+)\n\s+\.value_kind:\s+(\S+)", blk) if not kind.startswith("hidden")]
        assert sizes == want, sizes
    assert want[:4] == [16, 76, 412, 20]


def test_manipulator_unit_is_shipped_clean_or_refused_whole(tmp_path):
    """The dense five-link manipulator (n = 10, m = 3): either its train unit is as clean as the others', or the library refuses the WHOLE
    unit -- HJBX_EUNSUPPORTED naming the kernel and its bytes of scratch, the same error at once on the second call, a sane compile log --
    and the handle keeps its rollout unit; the controller then chooses autograd after one warning, and raises when fusion was
    demanded."""
    d = train_systems()["manip10"]()
    h = d.system
    assert h.param_grad and not fused_systems()["manip10"]().system.param_grad
    cfg = make_vhjb_config("nearhover")
    for act in ("relu", "tanh"):
        try:
            h.code_object(("train", act))
        except NotImplementedError as err:
            msg = str(err)
            assert re.search(r"k_train_coop<mode \d, PS \d> kernel .* needs \d+ bytes of scratch", msg), msg
            t0 = time.perf_counter()
            with pytest.raises(NotImplementedError) as again:
                h.code_object(("train", act))
            assert time.perf_counter() - t0 < 0.5 and str(again.value) == msg
            assert "error:" not in _abi.compile_log()
            assert _grad_rc(h, _fake_mlp(_abi._ACTIVATIONS[act]), 10, 3) == _abi.EUNSUPPORTED and "bytes of scratch" in _abi.last_error()
            assert h.code_object(("pd", act))[:4] == b"\x7fELF"                                   # the rollout unit of the same handle
            # the controller's decision (its constructor needs a device for the rest; tests/test_gpu_user_train.py builds one): automatic
            # mode warns once with the library's message and trains through autograd, a demanded fusion raises
            choose = lambda want: VHJBController._choose_fused_param_grad(d, cfg, torch.float32, act, False, torch.device("cuda"), want)
            with warnings.catch_warnings(record=True) as seen:
                warnings.simplefilter("always")
                assert choose(None) is False
            mine = [w for w in seen if "fused parameter gradient" in str(w.message)]
            assert len(mine) == 1 and "bytes of scratch" in str(mine[0].message)
            with pytest.raises(NotImplementedError, match="bytes of scratch"):
                choose(True)
            assert choose(False) is False
            # a system that did not ask with param_grad=True keeps autograd in automatic mode, silently and without a compile (as before)
            quiet = fused_systems()["manip10"]()
            with warnings.catch_warnings(record=True) as seen:
                warnings.simplefilter("always")
                t0 = time.perf_counter()
                assert VHJBController._choose_fused_param_grad(quiet, cfg, torch.float32, act, False, torch.device("cuda"), None) is False
            assert not seen and time.perf_counter() - t0 < 0.5
        else:
            _loaded_unit_is_clean(h, act, tmp_path, f"manip10_{act}")
    with pytest.raises(NotImplementedError, match="n <= 4"):
        h.code_object(("train", "sin"))


def test_user_train_unit_isa_audit(tmp_path):
    """The translation unit the library hands to hiprtc (hjbx_user_train_kernels.hpp around the user's snippet), compiled offline with the
    same flags: four kernels, no scratch, and both inline-asm audits of tools/audit_asm_loads.py clean -- every hand-scheduled ds_read of
    the chains is retired before the MFMA that consumes it, also around arbitrary user code."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import audit_asm_loads
    damped = CARTPOLE_SRC.replace("DAMP0", "p[4]").replace("DAMP1", "p[5]")
    cases = [("cartpole_tanh", damped, 4, 1, 6, 1, 1), ("cartpole_sin", damped, 4, 1, 6, 1, 2), ("quad2d_relu", QUAD2D_SRC, 6, 2, 4, 0, 0),
             ("quad2d_tanh", QUAD2D_SRC, 6, 2, 4, 0, 1)]
    procs = []
    for tag, src, n, m, npar, kind, act in cases:
        d = tmp_path / tag
        d.mkdir()
        (d / "hjbx_user_snippet.hpp").write_text(src)
        (d / "unit.hip").write_text('#include "hjbx_user_train_kernels.hpp"\n')
        asm = d / "unit.s"
        cmd = HIPCC + ["-S", "--cuda-device-only", f"-I{d}", f"-I{CSRC}", f"-DHJBX_USER_N={n}", f"-DHJBX_USER_M={m}", f"-DHJBX_USER_NP={npar}",
                       f"-DHJBX_USER_KIND={kind}", f"-DHJBX_USER_MLP_ACT={act}", "-o", str(asm), str(d / "unit.hip")]
        procs.append((tag, asm, subprocess.Popen(cmd, stderr=subprocess.DEVNULL)))
    for tag, asm, pr in procs:
        assert pr.wait() == 0, tag
        text = asm.read_text()
        kernels = META.findall(text)
        assert len(kernels) == 4 and all(KERNEL.match(k[0]) for k in kernels), (tag, [k[0] for k in kernels])
        assert "hjbx_u_affine_f32" not in text                                   # the streaming kernels are not compiled a second time
        for kname, private, _sgpr_spill, vgprs, vgpr_spill in kernels:
            assert int(private) == 0 and int(vgpr_spill) == 0 and int(vgprs) <= 512, (tag, kname, private, vgpr_spill, vgprs)
        assert audit_asm_loads.audit(str(asm)) == 0, tag
        assert audit_asm_loads.audit_mfma_asm_reads(str(asm)) == 0, tag


def _task(n, m):
    import numpy as np
    return _abi.make_task(n, m, np.eye(n), np.eye(m), None, np.zeros(n), np.zeros(m), None, None, 1e-7)


def _grad_rc(h, mlp, n, m):
    """hjbx_value_loss_grad_f32 with pointers the argument checks accept (the calls below never get as far as a launch)"""
    return _abi.lib().hjbx_value_loss_grad_f32(h.ptr, _abi.ref(_task(n, m)), _abi.ref(mlp), 0, 0x1000, 0x1000, 0x1000, 0x1000, 0x1000, 64, None)


def test_refusals_of_the_two_entry_points():
    L = _abi.lib()
    # a handle that did not ask: refused at once, nothing compiled, no train code object to read
    plain = UserQuad2D(D.quadrotors2d_dynamics_config()).system
    t0 = time.perf_counter()
    assert _grad_rc(plain, _fake_mlp(), 6, 2) == _abi.EUNSUPPORTED and "has not asked" in _abi.last_error()
    with pytest.raises(NotImplementedError, match="has not asked"):
        plain.code_object(("train", "relu"))
    assert time.perf_counter() - t0 < 0.5
    # an odd state dimension can never be enabled: the entry point says why
    odd = "HJBX_DEV void wrap(T* x) const {}\nHJBX_DEV void affine(const T* x, T* f1, T* f2) const { for (int i = 0; i < 3; ++i) { f1[i] = x[i]; f2[i] = T(1); } }\n"
    h3 = _abi.SystemHandle.from_source(_abi.USER_AFFINE, odd, 3, 1, 0.02, [-1], [1], [1.0])
    assert _grad_rc(h3, _fake_mlp(), 3, 1) == _abi.EUNSUPPORTED and "even state dimension" in _abi.last_error()
    with pytest.raises(NotImplementedError, match="even state dimension"):
        h3.code_object(("train", "relu"))
    # sin with n > 4, as for the built-in systems; nothing is compiled for it
    ok = FusedQuad2D(D.quadrotors2d_dynamics_config()).system
    t0 = time.perf_counter()
    assert _grad_rc(ok, _fake_mlp(_abi.ACT_SIN), 6, 2) == _abi.EUNSUPPORTED and "n <= 4" in _abi.last_error()
    # float32 MFMA arithmetic and the cooperative kernel only: both options are named
    for opt, name in ((_abi.OPT_MLP_ARITHMETIC, "HJBX_OPT_MLP_ARITHMETIC"), (_abi.OPT_TRAIN_KERNEL, "HJBX_OPT_TRAIN_KERNEL")):
        prev = _abi.set_option(opt, 1)
        try:
            assert _grad_rc(ok, _fake_mlp(), 6, 2) == _abi.EUNSUPPORTED and name in _abi.last_error()
            adam = _abi.HjbxAdamState()                                                           # an Adam state the entry point's own checks accept
            for i, numel in enumerate((6 * 128, 128 * 128, 128 * 64)):
                adam.param[i], adam.exp_avg[i], adam.exp_avg_sq[i], adam.step[i], adam.numel[i] = 0x1000, 0x2000, 0x3000, 0x4000, numel
            adam.ticket, adam.lr, adam.beta1, adam.beta2, adam.eps = 0x5000, 1e-3, 0.9, 0.999, 1e-8
            rc = L.hjbx_value_loss_adam_f32(ok.ptr, _abi.ref(_task(6, 2)), _abi.ref(_fake_mlp()), 0, 0x1000, 0x1000, 0x1000, None, 0.1, 1e-7, C.pointer(adam),
                                            None, None, None, None, 0x1000, 64, None)
            assert rc == _abi.EUNSUPPORTED and name in _abi.last_error() and "hjbx_value_loss_adam_f32" in _abi.last_error()
        finally:
            _abi.set_option(opt, prev)
    assert time.perf_counter() - t0 < 0.5
    # the argument checks of the entry point still come first for a user handle
    bad = _fake_mlp()
    bad.h1 = 64
    assert _grad_rc(ok, bad, 6, 2) == _abi.EUNSUPPORTED and "features" in _abi.last_error()


def test_a_compile_failure_of_the_train_unit_only():
    """A snippet that compiles into the streaming kernels and the rollout unit but not into the train unit (HJBX_USER_TRAIN_UNIT is defined
    there only): the compiler's message comes back, the failure is remembered, and the other units stay usable."""
    src = "#ifdef HJBX_USER_TRAIN_UNIT\n#error this snippet refuses the train unit\n#endif\n" + QUAD2D_SRC
    h = _abi.SystemHandle.from_source(_abi.USER_AFFINE, src, 6, 2, 0.05, [-1, -1], [1, 1], [0.5, 0.2, 0.1, 9.81])
    h.enable_matrix_cores()
    assert _grad_rc(h, _fake_mlp(), 6, 2) == _abi.EINVAL and "does not compile" in _abi.last_error()
    assert "this snippet refuses the train unit" in _abi.compile_log()
    t0 = time.perf_counter()
    with pytest.raises(ValueError, match="compiler log"):
        h.code_object(("train", "relu"))
    assert time.perf_counter() - t0 < 0.5
    assert "this snippet refuses the train unit" in _abi.compile_log()
    assert h.matrix_cores and h.code_object("streaming")[:4] == b"\x7fELF" and h.code_object(("pd", "relu"))[:4] == b"\x7fELF"


def test_header_and_bindings_declare_the_train_unit():
    hdr = open(os.path.join(ROOT, "include", "hjbx.h")).read()
    assert re.search(r"#define HJBX_HAS_USER_TRAIN 1\b", hdr)
    assert re.search(r"#define HJBX_CODE_TRAIN\(activation\) \(7 \+ \(activation\)\)", hdr) and _abi.CODE_TRAIN == 7
    assert int(re.search(r"#define HJBX_VERSION (\d+)", hdr).group(1)) == 112
    for entry, begins in (("hjbx_value_loss_grad_f32", "The parameter gradient of one value-learning step"),
                          ("hjbx_value_loss_adam_f32", "params_update (vhjb.py:255-288) in ONE call")):
        doc = hdr[hdr.index(begins):hdr.index(f"int {entry}(")]                                  # what the header says at this entry point
        assert "hjbx_system_enable_matrix_cores" in doc and "scratch" in doc and "HJBX_OPT_TRAIN_KERNEL" in doc, entry
    embedded = open(os.path.join(CSRC, "hjbx_user.hip")).read()
    # (one list of embedded headers: symbol, file, the name hiprtc sees; the .incbin lines and the arrays handed to hiprtc come from it)
    assert 'X(hjbx_src_train_coop, "hjbx_train_coop_kernels.hpp", "hjbx_train_coop_kernels.hpp")' in embedded
    assert "HJBX_EMBEDDED_HEADERS(HJBX_EMBED)" in embedded and "HJBX_EMBEDDED_HEADERS(HJBX_TEXT)" in embedded and "HJBX_EMBEDDED_HEADERS(HJBX_NAME)" in embedded
    unit = open(os.path.join(CSRC, "hjbx_user_train_kernels.hpp")).read()
    assert "#define HJBX_USER_MATRIX_CORE_UNIT 1" in unit and unit.count("template __global__ void HJBX_UT_") == 4


def test_builtin_instruction_streams_are_recorded_as_unchanged():
    """Hoisting k_train_coop into a header must not change a built-in kernel: tools/dev/coop_isa_equal.py compared llvm-objdump -d per
    k_train_coop symbol of libhjbx.so before and after, and profiles/user_train.json keeps the result."""
    with open(os.path.join(ROOT, "profiles", "user_train.json")) as f:
        prof = json.load(f)
    eq = prof["builtin_instruction_streams"]
    assert eq["identical"] is True and eq["differing"] == [] and eq["missing_after"] == []
    assert eq["k_train_coop_instantiations"] >= 5 * 2 * 2 * 2 and eq["instructions_compared"] > 100000
    assert "measured" in prof
