#!/usr/bin/env python3
"""Do the five Hessian units of two source trees compile to the same vector and matrix code?  Written for the fold of the two Hessian
kernels into one (k_value_hessian<S, WAVES, ACT, HEAD> of csrc/hjbx_hessian_kernels.hpp): the kernel arguments move, nothing else may.

Each unit (hjbx_hessian.hip x relu / tanh / sin, hjbx_softpd_hessian.hip x tanh / sin) is compiled from both trees with the flags of the
host tests (-S --cuda-device-only) and compared:
  * per instantiation (matched by its system): vgpr_count equal, private_segment_fixed_size 0 and vgpr_spill_count 0 on both sides;
  * per unit: the count of every instruction mnemonic that does not start with s_ equal; the scalar mnemonics that differ are listed.
No GPU needed.  Prints one JSON object (the `machine_code` block of profiles/hessian_host_refactor.json); exit status 1 when a vector or
matrix count, a register count or a kernel differs.

    python tools/dev/hessian_isa_counts.py <csrc of the parent commit> [<csrc of this tree>]
"""
import collections
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HIPCC = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=on", "-S", "--cuda-device-only"]
UNITS = [("hjbx_hessian.hip", f"-DHJBX_HESS_ACT={a}", f"pd_{n}") for a, n in enumerate(("relu", "tanh", "sin"))] + \
        [("hjbx_softpd_hessian.hip", f"-DHJBX_SOFTPD_HESS_ACT={a}", f"softpd_{n}") for a, n in ((1, "tanh"), (2, "sin"))]
META = re.compile(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.sgpr_count:\s+(\d+)\n(?:.*\n)*?"
                  r"\s+\.vgpr_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)")


def compile_all(csrc, tmp, tag):
    procs = []
    for src, define, name in UNITS:
        out = os.path.join(tmp, f"{tag}_{name}.s")
        procs.append((name, out, subprocess.Popen(HIPCC + [define, "-o", out, os.path.join(csrc, src)], stderr=subprocess.DEVNULL)))
    res = {}
    for name, out, pr in procs:
        if pr.wait() != 0:
            raise SystemExit(f"{csrc}: {name} does not compile")
        res[name] = open(out).read()
    return res


def digest(asm):
    """-> ({system: (vgprs, sgprs, scratch bytes, spilled VGPRs)}, {mnemonic: count}) of one unit"""
    code, _, meta = asm.partition(".amdgpu_metadata")
    kernels = {}
    for name, private, sgprs, vgprs, spill in META.findall(meta):
        system = re.search(r"hessianI(?:N4hjbx)?\d+(\w+?)If(?:Li(\d+))?", name)
        kernels[system.group(1) + (system.group(2) or "")] = (int(vgprs), int(sgprs), int(private), int(spill))
    return kernels, collections.Counter(re.findall(r"^\t([a-z][a-z0-9_]*)(?:\s|$)", code, flags=re.M))


def main():
    before_dir = sys.argv[1]
    after_dir = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "q_learning_with_hjb_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        before, after = compile_all(before_dir, tmp, "before"), compile_all(after_dir, tmp, "after")
    ok, units = True, {}
    for _, _, name in UNITS:
        (kb, cb), (ka, ca) = digest(before[name]), digest(after[name])
        same_kernels = sorted(kb) == sorted(ka) and len(ka) == 7
        clean = all(k[2] == 0 and k[3] == 0 for k in list(kb.values()) + list(ka.values()))
        vgprs_equal = same_kernels and all(kb[s][0] == ka[s][0] for s in kb)
        vector = {m: [cb[m], ca[m]] for m in sorted(set(cb) | set(ca)) if not m.startswith("s_") and cb[m] != ca[m]}
        scalar = {m: [cb[m], ca[m]] for m in sorted(set(cb) | set(ca)) if m.startswith("s_") and cb[m] != ca[m]}
        ok &= same_kernels and clean and vgprs_equal and not vector
        units[name] = dict(instantiations=len(ka), vgpr_count={s: ka[s][0] for s in sorted(ka)}, vgpr_count_equals_parent=vgprs_equal,
                           no_scratch_no_spill=clean, sgpr_count_changed={s: [kb[s][1], ka[s][1]] for s in sorted(kb) if same_kernels and kb[s][1] != ka[s][1]},
                           v_mfma=[sum(v for m, v in cb.items() if m.startswith("v_mfma")), sum(v for m, v in ca.items() if m.startswith("v_mfma"))],
                           instructions=[sum(cb.values()), sum(ca.values())],
                           non_scalar_instructions=[sum(v for m, v in cb.items() if not m.startswith("s_")), sum(v for m, v in ca.items() if not m.startswith("s_"))],
                           non_scalar_mnemonics_differing=vector, scalar_mnemonics_differing=scalar)
    print(json.dumps(dict(tool="tools/dev/hessian_isa_counts.py", flags=" ".join(HIPCC[1:]), columns="[parent, this tree]", identical_vector_and_matrix_code=ok,
                          units=units), indent=1))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
