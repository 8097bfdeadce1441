"""CPU-only tests of the matrix-core kernels for user-defined systems (hjbx_system_enable_matrix_cores, csrc/hjbx_user_mlp_kernels.hpp): a
`Dynamics` subclass whose device_source() says matrix_cores=True gets the two persistent MFMA kernels of the value network compiled for it
at first use.  Here, without a device: the opt-in and its refusals, the lazy compile of every (head, activation) for three systems and
what the compiled code objects hold (kernels, scratch, registers), the ISA audits of the unit, and a compile failure that only the
matrix-core unit has.  No compute call touches a GPU."""
import ctypes as C
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import ROOT, make_dynamics
from q_learning_with_hjb_amd import _abi
from q_learning_with_hjb_amd.configs import defaults as D
from q_learning_with_hjb_amd.dynamics.dynamics_basic import Dynamics
from test_gpu_user_system import CARTPOLE_SRC, CFG, QUAD2D_SRC, UserCartpole, UserQuad2D

CSRC = os.path.join(ROOT, "q_learning_with_hjb_amd", "csrc")
HIPCC = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=on"]
READELF = "/opt/rocm/llvm/bin/llvm-readelf"
OBJDUMP = "/opt/rocm/llvm/bin/llvm-objdump"
HEADS, ACTS = ("pd", "soft"), ("relu", "tanh", "sin")

# a dense five-link manipulator (n = 10, m = 3): every entry of M, C, G is populated, M is symmetric and diagonally dominant (p[0] + i on the
# diagonal, off-diagonals <= 0.1 p[1]), so the Gauss-Jordan elimination of the generic manipulator form runs on a full 5 x 5 matrix
MANIP10_SRC = r"""
    HJBX_DEV void wrap(T* x) const { x[1] = wrap_angle(x[1]); x[2] = wrap_angle(x[2]); }
    HJBX_DEV void get_M(const T* x, T* Mq) const {
        constexpr int D = N / 2;
        T s, c; sincos_t(x[1], &s, &c);
        for (int i = 0; i < D; ++i) for (int j = 0; j < D; ++j) Mq[i * D + j] = (i == j ? p[0] + T(i) : T(0.1) * c * p[1] / T(1 + i + j));
    }
    HJBX_DEV void get_C(const T* x, T* Cq) const {
        constexpr int D = N / 2;
        T s, c; sincos_t(x[2], &s, &c);
        for (int i = 0; i < D; ++i) for (int j = 0; j < D; ++j) Cq[i * D + j] = (i == j ? p[2] : -p[1] * x[D + j] * s);
    }
    HJBX_DEV void get_G(const T* x, T* Gq) const {
        constexpr int D = N / 2;
        T s, c; sincos_t(x[1], &s, &c);
        for (int i = 0; i < D; ++i) Gq[i] = p[3] * s * T(i);
    }
    HJBX_DEV void get_B(T* Bq) const { constexpr int D = N / 2; for (int i = 0; i < D * M; ++i) Bq[i] = (i % (M + 1) == 0) ? T(1) : T(0); }
"""
MANIP10_PARAMS = [2.0, 0.8, 0.3, 4.0]


class FusedCartpole(UserCartpole):
    """the user cart-pole of test_gpu_user_system.py asking for the matrix-core kernels"""

    def device_source(self):
        return dict(super().device_source(), matrix_cores=True)


class FusedQuad2D(UserQuad2D):
    def device_source(self):
        return dict(super().device_source(), matrix_cores=True)


class Manip10(Dynamics):
    """n = 10, m = 3 with the near-hover quadcopter's configuration (limits, dt, start distribution): only the dimensions matter here"""

    def device_source(self):
        return dict(kind="manipulator", source=MANIP10_SRC, params=MANIP10_PARAMS, matrix_cores=True)


def fused_systems():
    return {"cartpole_damped": lambda: FusedCartpole(D.cartpole_dynamics_config(**CFG), damping=(0.4, 0.05)),
            "quad2d": lambda: FusedQuad2D(D.quadrotors2d_dynamics_config()),
            "manip10": lambda: Manip10(D.near_hover_dynamics_config())}


META = re.compile(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.sgpr_spill_count:\s+(\d+)\n"
                  r"(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)")

# (system, head, activation) whose matrix-core unit the library refuses to ship because a kernel would spill registers to scratch
# (HJBX_EUNSUPPORTED at the first use): DESIGN.md 4.8 lists the same set.  None at the time of writing.
REFUSED = set()


def kernel_metadata(code, tmp_path, tag):
    assert code[:4] == b"\x7fELF"
    path = tmp_path / f"{tag}.co"
    path.write_bytes(code)
    notes = subprocess.run([READELF, "--notes", str(path)], capture_output=True, text=True, check=True).stdout
    return path, META.findall(notes)


@pytest.mark.parametrize("name", ["cartpole_damped", "quad2d", "manip10"])
def test_every_head_and_activation_compiles_lazily_without_spills(name, tmp_path):
    """Three systems x {relu, tanh, sin} x {PD, soft-PD}: enabling compiles nothing; code_object((head, act)) compiles that unit and returns
    an ELF with exactly the value-gradient kernel and the Euler / RK4 rollout kernels of that head for the user's struct, each without
    scratch, without spilled VGPRs and within the 256 registers two waves per SIMD leave; the streaming object holds no MFMA kernel."""
    t0 = time.perf_counter()
    d = fused_systems()[name]()
    t_create = time.perf_counter() - t0
    h = d.system
    assert h.kind == _abi.SYS_USER and h.matrix_cores
    _, stream = kernel_metadata(h.code_object("streaming"), tmp_path, "streaming")
    assert len(stream) == 32 and all(k[0].startswith("hjbx_u_") for k in stream)
    times = []
    for head in HEADS:
        for act in ACTS:
            t0 = time.perf_counter()
            if (name, head, act) in REFUSED:
                with pytest.raises(NotImplementedError, match="scratch"):
                    h.code_object((head, act))
                continue
            code = h.code_object((head, act))
            times.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            assert h.code_object((head, act)) == code and time.perf_counter() - t0 < 0.5        # compiled once per handle
            path, kernels = kernel_metadata(code, tmp_path, f"{head}_{act}")
            names = sorted(k[0] for k in kernels)
            assert len(names) == 3, names
            want_head = "MlpHeadSoft" if head == "soft" else "MlpHeadPd"
            assert sum("k_value_grad_mfma" in k for k in names) == 1 and sum("k_vhjb_rollout_mfma" in k for k in names) == 2
            assert all("UserSystem" in k and want_head in k for k in names)
            assert sum("k_vhjb_rollout_mfmaILi0E" in k for k in names) == 1 and sum("k_vhjb_rollout_mfmaILi1E" in k for k in names) == 1
            for kname, private, sgpr_spill, vgprs, vgpr_spill in kernels:
                print(f"    {name} {head} {act} {kname[:28]}: {vgprs} VGPRs, {sgpr_spill} spilled SGPRs, {private} bytes of scratch")
                assert int(private) == 0 and int(vgpr_spill) == 0, f"{kname}: {private} bytes of scratch, {vgpr_spill} spilled VGPRs"
                assert int(vgprs) <= 256, f"{kname}: {vgprs} VGPRs do not fit two waves per SIMD"
            # what will really be loaded holds the three MFMA chains of every kernel, forward and backward
            dis = subprocess.run([OBJDUMP, "-d", str(path)], capture_output=True, text=True, check=True).stdout
            assert dis.count("v_mfma_f32_32x32x2_f32") >= 3 * 700
    print(f"\n{name}: from_source {t_create:.1f} s; matrix-core units {min(times):.1f} .. {max(times):.1f} s each")


def _write_unit(tmp_path, tag, source):
    d = tmp_path / tag
    d.mkdir()
    (d / "hjbx_user_snippet.hpp").write_text(source)
    (d / "unit.hip").write_text('#include "hjbx_user_mlp_kernels.hpp"\n')
    return d


def test_user_matrix_core_unit_isa_audit(tmp_path):
    """The translation unit the library hands to hiprtc (hjbx_user_mlp_kernels.hpp around the user's snippet), compiled offline with the
    same flags: three kernels, no scratch, and both inline-asm audits of tools/audit_asm_loads.py clean -- every hand-scheduled ds_read is
    retired before the MFMA that consumes it, also around arbitrary user code."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import audit_asm_loads
    damped = CARTPOLE_SRC.replace("DAMP0", "p[4]").replace("DAMP1", "p[5]")
    cases = [("cartpole_tanh_pd", damped, 4, 1, 6, 1, 1, 0), ("quad2d_relu_pd", QUAD2D_SRC, 6, 2, 4, 0, 0, 0),
             ("manip10_sin_pd", MANIP10_SRC, 10, 3, 4, 1, 2, 0), ("cartpole_tanh_soft", damped, 4, 1, 6, 1, 1, 1),
             ("manip10_relu_soft", MANIP10_SRC, 10, 3, 4, 1, 0, 1)]
    procs = []
    for tag, src, n, m, npar, kind, act, soft in cases:
        d = _write_unit(tmp_path, tag, src)
        asm = d / "unit.s"
        cmd = HIPCC + ["-S", "--cuda-device-only", f"-I{d}", f"-I{CSRC}", f"-DHJBX_USER_N={n}", f"-DHJBX_USER_M={m}", f"-DHJBX_USER_NP={npar}",
                       f"-DHJBX_USER_KIND={kind}", f"-DHJBX_USER_MLP_ACT={act}", f"-DHJBX_USER_MLP_SOFT={soft}", "-o", str(asm), str(d / "unit.hip")]
        procs.append((tag, asm, subprocess.Popen(cmd, stderr=subprocess.DEVNULL)))
    for tag, asm, pr in procs:
        assert pr.wait() == 0, tag
        text = asm.read_text()
        kernels = META.findall(text)
        assert len(kernels) == 3 and sum("k_vhjb_rollout_mfma" in k[0] for k in kernels) == 2, (tag, [k[0] for k in kernels])
        assert "hjbx_u_affine_f32" not in text                                   # the streaming kernels are not compiled a second time
        for kname, private, _sgpr_spill, vgprs, vgpr_spill in kernels:
            assert int(private) == 0 and int(vgpr_spill) == 0 and int(vgprs) <= 256, (tag, kname, private, vgpr_spill, vgprs)
        assert text.count("v_mfma_f32_32x32x2_f32") >= 3 * 700, tag
        assert audit_asm_loads.audit(str(asm)) == 0, tag
        assert audit_asm_loads.audit_mfma_asm_reads(str(asm)) == 0, tag


def _fake_mlp(act=_abi.ACT_RELU):
    """a descriptor the entry points accept up to the point where they would launch (the calls below never get that far)"""
    m = _abi.HjbxMlp()
    m.W1 = m.W2 = m.W3 = 0x1000
    m.h1, m.h2, m.h3, m.activation = 128, 128, 64, act
    for k in range(_abi.HJBX_MAX_N):
        m.mean[k], m.std[k], m.xf[k] = 0.0, 1.0, 0.0
    return m


def test_refusals_and_a_compile_failure_of_the_matrix_core_unit_only():
    L = _abi.lib()
    # an odd state dimension: the kernels walk the state in k-steps of 2
    odd = "HJBX_DEV void wrap(T* x) const {}\nHJBX_DEV void affine(const T* x, T* f1, T* f2) const { for (int i = 0; i < 3; ++i) { f1[i] = x[i]; f2[i] = T(1); } }\n"
    h3 = _abi.SystemHandle.from_source(_abi.USER_AFFINE, odd, 3, 1, 0.02, [-1], [1], [1.0])
    with pytest.raises(NotImplementedError, match="even"):
        h3.enable_matrix_cores()
    assert not h3.matrix_cores

    class Odd(Dynamics):
        def device_source(self):
            return dict(kind="affine", source=odd, params=[1.0], matrix_cores=True)
    cfg = D.cartpole_dynamics_config(**CFG)
    cfg.state_dim = 3
    cfg.x0_mean, cfg.x0_std = cfg.x0_mean[:3], cfg.x0_std[:3]
    with pytest.raises(NotImplementedError, match="even"):
        Odd(cfg)
    # a built-in system has its kernels in the library
    with pytest.raises(ValueError, match="built-in"):
        make_dynamics("cartpole").system.enable_matrix_cores()
    assert not make_dynamics("cartpole").system.matrix_cores
    with pytest.raises(ValueError):
        make_dynamics("cartpole").system.code_object("streaming")

    # a handle that did not ask: the entry point refuses at once (nothing is compiled), and there is no matrix-core code object to read
    plain = UserQuad2D(D.quadrotors2d_dynamics_config()).system
    assert not plain.matrix_cores
    mlp = _fake_mlp()
    t0 = time.perf_counter()
    rc = L.hjbx_value_grad_f32(plain.ptr, _abi.ref(mlp), 0x1000, 0x1000, 0x1000, 64, None)
    assert rc == _abi.EUNSUPPORTED and time.perf_counter() - t0 < 0.5
    with pytest.raises(NotImplementedError):
        _abi.check(rc)
    t0 = time.perf_counter()
    with pytest.raises(NotImplementedError, match="has not asked"):
        plain.code_object(("pd", "relu"))
    assert time.perf_counter() - t0 < 0.5
    assert plain.code_object("streaming")[:4] == b"\x7fELF"

    # a snippet that compiles into the streaming kernels but not into the matrix-core unit (HJBX_USER_MATRIX_CORE_UNIT is defined there
    # only): creation and enabling succeed, the lazy compile fails with the compiler's log, and the handle stays usable
    src = "#ifdef HJBX_USER_MATRIX_CORE_UNIT\n#error this snippet refuses the matrix-core unit\n#endif\n" + QUAD2D_SRC
    h = _abi.SystemHandle.from_source(_abi.USER_AFFINE, src, 6, 2, 0.05, [-1, -1], [1, 1], [0.5, 0.2, 0.1, 9.81])
    h.enable_matrix_cores()
    assert h.matrix_cores
    rc = L.hjbx_value_grad_f32(h.ptr, _abi.ref(mlp), 0x1000, 0x1000, 0x1000, 64, None)   # fails in the compile, before any launch
    assert rc == _abi.EINVAL and "does not compile" in _abi.last_error()
    assert "this snippet refuses the matrix-core unit" in _abi.compile_log()
    t0 = time.perf_counter()
    with pytest.raises(ValueError, match="compiler log"):
        h.code_object(("pd", "relu"))
    assert time.perf_counter() - t0 < 0.5                                               # the refusal is remembered, not compiled again
    assert "this snippet refuses the matrix-core unit" in _abi.compile_log()
    assert h.matrix_cores and h.code_object("streaming")[:4] == b"\x7fELF"
    n, m = C.c_int(), C.c_int()
    assert L.hjbx_dims(h.ptr, C.byref(n), C.byref(m)) == 0 and (n.value, m.value) == (6, 2)

    # the split arithmetics are not compiled for user systems: the PD entry points name the option
    ok = FusedQuad2D(D.quadrotors2d_dynamics_config()).system
    prev = _abi.set_option(_abi.OPT_MLP_ARITHMETIC, 1)
    try:
        rc = L.hjbx_value_grad_f32(ok.ptr, _abi.ref(mlp), 0x1000, 0x1000, 0x1000, 64, None)
        assert rc == _abi.EUNSUPPORTED and "HJBX_OPT_MLP_ARITHMETIC" in _abi.last_error()
    finally:
        _abi.set_option(_abi.OPT_MLP_ARITHMETIC, prev)


def test_header_declares_the_new_entry_points():
    hdr = open(os.path.join(ROOT, "include", "hjbx.h")).read()
    assert re.search(r"#define HJBX_HAS_USER_MATRIX_CORES 1\b", hdr)
    for name in ("hjbx_system_enable_matrix_cores", "hjbx_system_matrix_cores", "hjbx_system_code_object"):
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(_abi.lib(), name)
        assert re.search(rf"^(?:int|size_t) {name}\(", hdr, flags=re.M)
    assert int(re.search(r"#define HJBX_VERSION (\d+)", hdr).group(1)) == 112
    assert np.array_equal([1 + 3 * _abi._HEADS[h] + _abi._ACTIVATIONS[a] for h in HEADS for a in ACTS], np.arange(1, 7))
