"""CPU-only tests of the value-network Hessian for user-defined systems (csrc/hjbx_user_hessian_kernels.hpp): a handle that asked for the
matrix-core kernels gets k_value_hessian compiled for its struct at the first hjbx_value_hessian_f32 / hjbx_softpd_value_hessian_f32 call,
one unit per (head, activation).  Here, without a device: the lazy compile and what the code objects hold (one kernel, no scratch, no spilled
VGPR, the MFMA chains) at n = 4, 6, 8 and 10 -- n = 8 fills all 32 columns of a tile, which no built-in system does --, the ISA audits of
the unit compiled offline, the scratch refusal on a snippet made to need private memory, the argument checks in their order, and the header.
No compute call touches a GPU."""
import os
import re
import subprocess
import sys
import time

import pytest

from conftest import ROOT
from q_learning_with_hjb_amd import _abi
from q_learning_with_hjb_amd.configs import defaults as D
from test_gpu_user_system import QUAD2D_SRC, UserQuad2D
from test_user_fused_host import CSRC, HIPCC, MANIP10_SRC, META, OBJDUMP, fused_systems, kernel_metadata

# an affine system of eight states, two of them angles (coordinates 1 and 2): four damped oscillators, two inputs; p = stiffness, damping, gain
N8_SRC = r"""
    HJBX_DEV void wrap(T* x) const { x[1] = wrap_angle(x[1]); x[2] = wrap_angle(x[2]); }
    HJBX_DEV void affine(const T* x, T* f1, T* f2) const {
        for (int i = 0; i < 4; ++i) { f1[i] = x[4 + i]; f1[4 + i] = -p[0] * x[i] - p[1] * x[4 + i]; }
        for (int i = 0; i < 16; ++i) f2[i] = T(0);
        for (int i = 0; i < 4; ++i) f2[(4 + i) * 2 + (i & 1)] = p[2];
    }
"""
N8_PARAMS = [1.0, 0.5, 2.0]

# the planar quadrotor with a wrap that, in the Hessian unit only, goes through a local array indexed at run time: private memory, so scratch
SCRATCH_SRC = QUAD2D_SRC.replace("HJBX_DEV void wrap(T* x) const { x[2] = wrap_angle(x[2]); }", r"""HJBX_DEV void wrap(T* x) const {
#ifdef HJBX_USER_HESSIAN_UNIT
        T t[256];
        for (int i = 0; i < 256; ++i) t[i] = T(i);
        t[(int)(x[0] * T(16)) & 255] = x[2];
        x[2] = wrap_angle(x[2]) + T(0) * t[(int)(x[1] * T(16)) & 255];
#else
        x[2] = wrap_angle(x[2]);
#endif
    }""")
assert SCRATCH_SRC != QUAD2D_SRC

_handles = {}


def n8_handle():
    h = _abi.SystemHandle.from_source(_abi.USER_AFFINE, N8_SRC, 8, 2, 0.02, [-1, -1], [1, 1], N8_PARAMS)
    h.enable_matrix_cores()
    return h


def handle(name):
    """one enabled handle per system for the whole file: a unit is compiled once per handle"""
    if name not in _handles:
        if name == "n8":
            _handles[name] = (None, n8_handle())
        else:
            d = fused_systems()[name]()
            _handles[name] = (d, d.system)       # (the Dynamics owns the handle)
    return _handles[name][1]


# (system, head, activation): each head and each activation at n = 8 and at n = 10, one pair at n = 4 and at n = 6
UNITS = [("n8", "pd", "relu"), ("n8", "pd", "sin"), ("n8", "soft", "tanh"),
         ("manip10", "pd", "tanh"), ("manip10", "soft", "sin"), ("manip10", "pd", "relu"),
         ("cartpole_damped", "pd", "tanh"), ("quad2d", "soft", "sin")]


@pytest.mark.parametrize("name, head, act", UNITS, ids=["-".join(u) for u in UNITS])
def test_hessian_unit_compiles_lazily_into_one_clean_kernel(name, head, act, tmp_path):
    h = handle(name)
    assert h.kind == _abi.SYS_USER and h.matrix_cores
    t0 = time.perf_counter()
    code = h.code_object(("hessian", head, act))
    t_compile = time.perf_counter() - t0
    t0 = time.perf_counter()
    assert h.code_object(("hessian", head, act)) == code and time.perf_counter() - t0 < 0.5          # compiled once per handle
    path, kernels = kernel_metadata(code, tmp_path, f"hess_{head}_{act}")
    assert len(kernels) == 1, [k[0] for k in kernels]
    kname, private, sgpr_spill, vgprs, vgpr_spill = kernels[0]
    print(f"\n    {name} (n={h.n}) {head} {act}: {vgprs} VGPRs, {sgpr_spill} spilled SGPRs, {private} bytes of scratch, compiled in {t_compile:.1f} s")
    assert "k_value_hessian" in kname and "UserSystem" in kname and ("MlpHeadSoft" if head == "soft" else "MlpHeadPd") in kname, kname
    assert int(private) == 0 and int(vgpr_spill) == 0, f"{kname}: {private} bytes of scratch, {vgpr_spill} spilled VGPRs"
    assert int(vgprs) <= 512
    dis = subprocess.run([OBJDUMP, "-d", str(path)], capture_output=True, text=True, check=True).stdout
    assert dis.count("v_mfma_f32_32x32x2_f32") >= (1024 if act == "relu" else 1536)


def test_the_other_units_of_the_handle_are_untouched(tmp_path):
    """the Hessian kernel is a code object of its own: the matrix-core unit keeps its three kernels, the streaming object its 32"""
    h = handle("n8")
    hess = h.code_object(("hessian", "pd", "relu"))
    _, mc = kernel_metadata(h.code_object(("pd", "relu")), tmp_path, "mc")
    assert len(mc) == 3 and not any("k_value_hessian" in k[0] for k in mc), [k[0] for k in mc]
    _, stream = kernel_metadata(h.code_object("streaming"), tmp_path, "streaming")
    assert len(stream) == 32 and all(k[0].startswith("hjbx_u_") for k in stream)
    assert h.code_object(("hessian", "pd", "relu")) == hess


def test_user_hessian_unit_isa_audit(tmp_path):
    """The translation unit the library hands to hiprtc, compiled offline with the same flags: one kernel, no scratch, the streaming kernels
    not emitted again, and both inline-asm audits of tools/audit_asm_loads.py clean around the user's code."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import audit_asm_loads
    cases = [("n8_sin_pd", N8_SRC, 8, 2, 3, 0, 2, 0), ("manip10_sin_soft", MANIP10_SRC, 10, 3, 4, 1, 2, 1)]
    procs = []
    for tag, src, n, m, npar, kind, act, soft in cases:
        d = tmp_path / tag
        d.mkdir()
        (d / "hjbx_user_snippet.hpp").write_text(src)
        (d / "unit.hip").write_text('#include "hjbx_user_hessian_kernels.hpp"\n')
        asm = d / "unit.s"
        cmd = HIPCC + ["-S", "--cuda-device-only", f"-I{d}", f"-I{CSRC}", f"-DHJBX_USER_N={n}", f"-DHJBX_USER_M={m}", f"-DHJBX_USER_NP={npar}",
                       f"-DHJBX_USER_KIND={kind}", f"-DHJBX_USER_MLP_ACT={act}", f"-DHJBX_USER_MLP_SOFT={soft}", "-o", str(asm), str(d / "unit.hip")]
        procs.append((tag, asm, subprocess.Popen(cmd, stderr=subprocess.DEVNULL)))
    for tag, asm, pr in procs:
        assert pr.wait() == 0, tag
        text = asm.read_text()
        kernels = META.findall(text)
        assert len(kernels) == 1 and "k_value_hessian" in kernels[0][0] and "UserSystem" in kernels[0][0], (tag, [k[0] for k in kernels])
        assert "hjbx_u_affine_f32" not in text
        kname, private, _sgpr_spill, vgprs, vgpr_spill = kernels[0]
        assert int(private) == 0 and int(vgpr_spill) == 0 and int(vgprs) <= 512, (tag, kname, private, vgpr_spill, vgprs)
        assert text.count("v_mfma_f32_32x32x2_f32") >= 1536, tag
        assert audit_asm_loads.audit(str(asm)) == 0, tag
        assert audit_asm_loads.audit_mfma_asm_reads(str(asm)) == 0, tag
    # a soft-PD ReLU unit does not exist
    d = tmp_path / "n8_sin_pd"
    cmd = HIPCC + ["-S", "--cuda-device-only", f"-I{d}", f"-I{CSRC}", "-DHJBX_USER_N=8", "-DHJBX_USER_M=2", "-DHJBX_USER_NP=3", "-DHJBX_USER_KIND=0",
                   "-DHJBX_USER_MLP_ACT=0", "-DHJBX_USER_MLP_SOFT=1", "-o", str(d / "none.s"), str(d / "unit.hip")]
    pr = subprocess.run(cmd, capture_output=True, text=True)
    assert pr.returncode != 0 and "there is no soft-PD ReLU unit" in pr.stderr


def test_a_unit_that_needs_scratch_is_refused_and_the_refusal_remembered(tmp_path):
    """Nothing is launched here.  The kernel of SCRATCH_SRC needs private memory in the Hessian unit only: that unit is refused, at once again
    on the second request, and the handle keeps its matrix-core unit."""
    h = _abi.SystemHandle.from_source(_abi.USER_AFFINE, SCRATCH_SRC, 6, 2, 0.05, [-1, -1], [1, 1], [0.5, 0.2, 0.1, 9.81])
    h.enable_matrix_cores()
    with pytest.raises(NotImplementedError, match="scratch") as ei:
        h.code_object(("hessian", "pd", "tanh"))
    assert "value-Hessian" in str(ei.value) and "the 512 registers of the Hessian kernel" in str(ei.value)
    t0 = time.perf_counter()
    with pytest.raises(NotImplementedError, match="scratch"):
        h.code_object(("hessian", "pd", "tanh"))
    assert time.perf_counter() - t0 < 0.5
    # the entry point reports the remembered refusal (made-up addresses: the call ends in the unit, before any launch)
    rc, msg = _call(WHO_PD, h, act=_abi.ACT_TANH)
    assert rc == _abi.EUNSUPPORTED and "scratch" in msg and "value-Hessian" in msg, msg
    _, mc = kernel_metadata(h.code_object(("pd", "tanh")), tmp_path, "mc")
    assert len(mc) == 3 and all(int(k[1]) == 0 for k in mc)
    assert h.matrix_cores and h.code_object("streaming")[:4] == b"\x7fELF"


# ------------------------------------------------------------------------------------------------------------------------------------
# argument checks (made-up addresses, as in test_value_hessian_host.py: every call comes back before the device is touched)
# ------------------------------------------------------------------------------------------------------------------------------------
PTR = 0x7F0000100000
ADDR = {name: PTR + 0x10000 * k for k, name in enumerate(("x", "H", "dy", "W1", "W2", "W3", "b1", "b2", "b3", "w4", "b4"))}
WHO_PD, WHO_SOFT = "hjbx_value_hessian_f32", "hjbx_softpd_value_hessian_f32"
USER = "user-defined systems are not supported"
ALIGN_PD = "x must be aligned to its row vector width, H and dy_dx to 16 bytes"
ALIGN_SOFT = "x must be aligned to its row vector width, H to 16 bytes"


def _call(who, h, act=_abi.ACT_TANH, edit=None, **over):
    soft = who == WHO_SOFT
    d = _abi.HjbxSoftpdMlp() if soft else _abi.HjbxMlp()
    for k in ("W1", "W2", "W3") + (("b1", "b2", "b3", "w4", "b4") if soft else ()):
        setattr(d, k, ADDR[k])
    d.h1, d.h2, d.h3, d.activation = 128, 128, 64, act
    for k in range(h.n):
        d.std[k] = 1.0
    if edit:
        edit(d)
    a = dict(ADDR, B=64)
    a.update(over)
    L = _abi.lib()
    if soft:
        rc = L.hjbx_softpd_value_hessian_f32(h.ptr, _abi.ref(d), a["x"], a["H"], a["B"], None)
    else:
        rc = L.hjbx_value_hessian_f32(h.ptr, _abi.ref(d), a["x"], a["H"], a["dy"], a["B"], None)
    return rc, _abi.last_error()


def _features(d):
    d.h2 = 64


def _std_zero(d):
    d.std[3] = 0.0


@pytest.mark.parametrize("who", [WHO_PD, WHO_SOFT])
def test_argument_checks_keep_their_order_for_a_user_handle(who):
    plain = UserQuad2D(D.quadrotors2d_dynamics_config()).system
    assert not plain.matrix_cores
    align = ALIGN_SOFT if who == WHO_SOFT else ALIGN_PD
    # a handle that has not asked: refused after the NULL-pointer check and before the features
    for kw in (dict(), dict(edit=_features)):
        rc, msg = _call(who, plain, **kw)
        assert rc == _abi.EUNSUPPORTED and USER in msg and "hjbx_system_enable_matrix_cores" in msg and msg.startswith(who + ": "), msg
    rc, msg = _call(who, plain, x=None)
    assert rc == _abi.EINVAL and "NULL x" in msg, msg
    # an enabled handle passes that point: features, alignment, std == 0 in the existing order with the existing messages
    t0 = time.perf_counter()
    h = n8_handle()            # (its own handle: nothing below may compile a unit)
    t_create = time.perf_counter() - t0
    t0 = time.perf_counter()
    rc, msg = _call(who, h, x=None)
    assert rc == _abi.EINVAL and "NULL x" in msg, msg
    rc, msg = _call(who, h, edit=_features)
    assert rc == _abi.EUNSUPPORTED and "features must be [128,128,64], got [128,64,64]" in msg, msg
    rc, msg = _call(who, h, act=7)
    assert rc == _abi.EINVAL and "unknown activation 7" in msg, msg
    rc, msg = _call(who, h, x=ADDR["x"] + 8)
    assert rc == _abi.EINVAL and align in msg, msg
    rc, msg = _call(who, h, x=ADDR["x"] + 8, edit=_std_zero)
    assert rc == _abi.EINVAL and align in msg, msg
    rc, msg = _call(who, h, H=ADDR["H"] + 8)
    assert rc == _abi.EINVAL and align in msg, msg
    rc, msg = _call(who, h, edit=_std_zero)
    assert rc == _abi.EINVAL and "normalization_std[3] is zero" in msg and msg.startswith(who + ": "), msg
    # nothing to compute: OK, and nothing is compiled
    for kw in (dict(B=0), dict(H=None, dy=None), dict(B=0, x=None)):
        rc, msg = _call(who, h, **kw)
        assert rc == _abi.OK, msg
    assert time.perf_counter() - t0 < 0.5, f"a unit was compiled (creating the handle took {t_create:.1f} s)"


def test_code_hessian_refusals():
    h = n8_handle()
    plain = UserQuad2D(D.quadrotors2d_dynamics_config()).system
    t0 = time.perf_counter()
    with pytest.raises(NotImplementedError, match="identically zero"):
        h.code_object(("hessian", "soft", "relu"))
    with pytest.raises(NotImplementedError, match="has not asked for the matrix-core kernels"):
        plain.code_object(("hessian", "pd", "tanh"))
    assert _abi.lib().hjbx_system_code_object(h.ptr, 16, None, 0) == 0 and "unknown code object 16" in _abi.last_error()
    assert time.perf_counter() - t0 < 0.5      # no unit is compiled for a refusal


def test_header_and_build_lists():
    hdr = open(os.path.join(ROOT, "include", "hjbx.h")).read()
    assert re.search(r"^#define HJBX_HAS_USER_VALUE_HESSIAN 1\b", hdr, flags=re.M)
    assert re.search(r"^#define HJBX_CODE_HESSIAN\(head, activation\) \(10 \+ 3 \* \(head\) \+ \(activation\)\)", hdr, flags=re.M)
    assert int(re.search(r"#define HJBX_VERSION (\d+)", hdr).group(1)) == 112 and _abi.lib().hjbx_version() == 112
    assert _abi.CODE_HESSIAN == 10
    assert "hjbx_user_hessian_kernels.hpp" in _abi._HEADERS and "hjbx_hessian_kernels.hpp" in _abi._HEADERS
    user_hip = open(os.path.join(CSRC, "hjbx_user.hip")).read()
    for name in ("hjbx_hessian_kernels.hpp", "hjbx_user_hessian_kernels.hpp"):
        assert re.search(rf'X\(\w+, "{re.escape(name)}", "{re.escape(name)}"\)', user_hip), name
    unit = open(os.path.join(CSRC, "hjbx_user_hessian_kernels.hpp")).read()
    assert "#define HJBX_USER_MATRIX_CORE_UNIT 1" in unit and "#define HJBX_USER_HESSIAN_UNIT 1" in unit
    assert len(re.findall(r"^template __global__", unit, flags=re.M)) == 1 and "HJBX_UH_VALUE_HESSIAN" in unit
