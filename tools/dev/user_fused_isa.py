#!/usr/bin/env python3
"""ISA comparison of the matrix-core kernels compiled for user-defined systems (csrc/hjbx_user_mlp_kernels.hpp) with the built-in
instantiations of the same (N, M): per kernel .sgpr_spill_count, .vgpr_count, scratch, and the number of v_readlane / v_writelane INSIDE the
MFMA chains.  No GPU needed (hipcc -S --cuda-device-only; --loaded adds the code objects libhjbx.so compiles through hiprtc); prints a JSON
object (the `isa` block of profiles/user_fused.json).

"Inside a chain": a chain is a run of v_mfma instructions whose gaps hold only what issues beside the matrix pipe (ds_read, s_waitcnt, a few
s_nop); every gap between two consecutive MFMAs with fewer than GAP other instructions counts as inside a chain, and the lane operations found
in such gaps are counted.  (The element-wise passes between the chains are hundreds of instructions long.)

    python tools/dev/user_fused_isa.py [--act 0] [--loaded] > isa.json
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CSRC = os.path.join(ROOT, "q_learning_with_hjb_amd", "csrc")
HIPCC = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=on", "-S", "--cuda-device-only"]
GAP = 24
sys.path.insert(0, os.path.join(ROOT, "tests"))


def functions(text):
    """-> {symbol: [instruction lines]} of an AMDGPU assembly file"""
    out, name, body = {}, None, []
    for line in text.splitlines():
        m = re.match(r"^(\w+):\s*(;.*)?$", line)
        if m and not line.startswith(".L"):
            name, body = m.group(1), []
            out[name] = body
        elif name and line.startswith("\t") and not line.lstrip().startswith((".", ";")):
            body.append(line.strip())
        if line.startswith("\t.end_amdhsa_kernel") or line.lstrip().startswith(".Lfunc_end"):
            name = None
    return out


def chain_lane_ops(body):
    idx = [k for k, ins in enumerate(body) if ins.startswith("v_mfma")]
    inside = 0
    for a, b in zip(idx, idx[1:]):
        if b - a - 1 < GAP:
            inside += sum(ins.startswith(("v_readlane", "v_writelane")) for ins in body[a + 1:b])
    total = sum(ins.startswith(("v_readlane", "v_writelane")) for ins in body)
    return dict(mfma=len(idx), lane_ops_inside_chains=inside, lane_ops_total=total)


META = re.compile(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.sgpr_count:\s+(\d+)\n(?:.*\n)*?\s+\.sgpr_spill_count:\s+(\d+)\n"
                  r"(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)")


def summarize(text, keep):
    fn = functions(text)
    rows = {}
    for name, private, sgprs, sgpr_spill, vgprs, vgpr_spill in META.findall(text):
        label = keep(name)
        if label:
            rows[label] = dict(scratch_bytes=int(private), sgpr_count=int(sgprs), sgpr_spill_count=int(sgpr_spill), vgpr_count=int(vgprs),
                               vgpr_spill_count=int(vgpr_spill), **chain_lane_ops(fn.get(name, [])))
    return rows


def disassembled_functions(path):
    """-> {symbol: [instruction lines]} of llvm-objdump -d on a code object"""
    out, body = {}, None
    for line in subprocess.run(["/opt/rocm/llvm/bin/llvm-objdump", "-d", path], capture_output=True, text=True, check=True).stdout.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
        if m:
            body = out.setdefault(m.group(1), [])
        elif body is not None and line.startswith("\t"):
            body.append(line.split("//")[0].strip())
    return out


def loaded_objects(act):
    """The code objects the library itself compiles (hiprtc) for the same three systems: what a GPU really loads."""
    from test_user_fused_host import fused_systems
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for tag, mk in fused_systems().items():
            path = os.path.join(tmp, tag + ".co")
            open(path, "wb").write(mk().system.code_object(("pd", ["relu", "tanh", "sin"][act])))
            notes = subprocess.run(["/opt/rocm/llvm/bin/llvm-readelf", "--notes", path], capture_output=True, text=True, check=True).stdout
            fn = disassembled_functions(path)
            rows = {}
            for name, private, sgprs, sgpr_spill, vgprs, vgpr_spill in META.findall(notes):
                rows[kind_of(name)] = dict(scratch_bytes=int(private), sgpr_count=int(sgprs), sgpr_spill_count=int(sgpr_spill), vgpr_count=int(vgprs),
                                           vgpr_spill_count=int(vgpr_spill), **chain_lane_ops(fn.get(name, [])))
            res["hiprtc_" + tag] = rows
    return res


def kind_of(name):
    if "k_value_grad_mfma" in name:
        return "value_grad"
    m = re.search(r"k_vhjb_rollout_mfmaILi(\d)E", name)
    return {"0": "rollout_euler", "1": "rollout_rk4"}.get(m.group(1)) if m else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--act", type=int, default=0, help="hjbx_activation: 0 relu, 1 tanh, 2 sin")
    ap.add_argument("--loaded", action="store_true", help="also the code objects libhjbx.so compiles through hiprtc (needs the built library)")
    a = ap.parse_args()
    from test_gpu_user_system import CARTPOLE_SRC, QUAD2D_SRC
    from test_user_fused_host import MANIP10_SRC
    users = {"user_cartpole_n4_m1": (CARTPOLE_SRC.replace("DAMP0", "p[4]").replace("DAMP1", "p[5]"), 4, 1, 6, 1),
             "user_quad2d_n6_m2": (QUAD2D_SRC, 6, 2, 4, 0), "user_manip10_n10_m3": (MANIP10_SRC, 10, 3, 4, 1)}
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        procs = []
        for tag, (src, n, m, npar, kind) in users.items():
            d = os.path.join(tmp, tag)
            os.makedirs(d)
            open(os.path.join(d, "hjbx_user_snippet.hpp"), "w").write(src)
            open(os.path.join(d, "unit.hip"), "w").write('#include "hjbx_user_mlp_kernels.hpp"\n')
            cmd = HIPCC + [f"-I{d}", f"-I{CSRC}", f"-DHJBX_USER_N={n}", f"-DHJBX_USER_M={m}", f"-DHJBX_USER_NP={npar}", f"-DHJBX_USER_KIND={kind}",
                           f"-DHJBX_USER_MLP_ACT={a.act}", "-DHJBX_USER_MLP_SOFT=0", "-o", os.path.join(d, "unit.s"), os.path.join(d, "unit.hip")]
            procs.append((tag, os.path.join(d, "unit.s"), subprocess.Popen(cmd, stderr=subprocess.DEVNULL)))
        mlp_act = {0: 0, 1: 1, 2: 4}[a.act]
        builtin_s = os.path.join(tmp, "builtin.s")
        procs.append(("builtin", builtin_s, subprocess.Popen(HIPCC + [f"-DHJBX_MLP_ACT={mlp_act}", "-o", builtin_s, os.path.join(CSRC, "hjbx_mlp.hip")],
                                                           stderr=subprocess.DEVNULL)))
        for tag, path, pr in procs:
            if pr.wait() != 0:
                raise SystemExit(f"{tag}: hipcc failed")
            text = open(path).read()
            if tag == "builtin":
                for sysname, label in (("8CartpoleIfE", "builtin_cartpole_n4_m1"), ("6Quad2DIfE", "builtin_quad2d_n6_m2"), ("9NearHoverIfE", "builtin_nearhover_n10_m3")):
                    res[label] = summarize(text, lambda nm, s=sysname: kind_of(nm) if s in nm and "Li2EN4hjbx" not in nm[:40] else None)
            else:
                res[tag] = summarize(text, kind_of)
    if a.loaded:
        res.update(loaded_objects(a.act))
    json.dump(dict(activation=["relu", "tanh", "sin"][a.act], chain_gap_threshold=GAP, kernels=res), sys.stdout, indent=1, sort_keys=True)
    print()


if __name__ == "__main__":
    main()
