#!/usr/bin/env python3
"""Are the k_train_coop instruction streams of two builds of libhjbx.so the same?  Written for the hoist of the kernel's device code into
csrc/hjbx_train_coop_kernels.hpp (so that hiprtc can compile it for a user-defined system): the built-in instantiations must not change.

Every gfx950 code object is taken out of the two libraries' .hip_fatbin bundles, disassembled with llvm-objdump -d, and the instructions
(mnemonics and operands; addresses, encodings and the `// ...` annotations dropped) compared per symbol whose name contains `k_train_coop`
(the main kernel of every system / mode / activation / PS, and the reduce / update epilogues).  No GPU needed.  Prints one JSON object (the
`builtin_instruction_streams` block of profiles/user_train.json); exit status 1 when a stream differs or a symbol of the first library is missing from the second
(symbols only the second has are listed, not compared).

--filter SUBSTRING (repeatable) compares the symbols whose name contains one of the substrings instead, e.g. k_value_grad_mfma,
k_vhjb_rollout_mfma, k_train_ for a change of the host code around those kernels.

    python tools/dev/coop_isa_equal.py [--filter SUBSTRING ...] <libhjbx.so of the parent commit> [<libhjbx.so of this tree>]
"""
import argparse
import hashlib
import json
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OBJDUMP = "/opt/rocm/llvm/bin/llvm-objdump"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(lib):
    """-> the gfx950 ELF images inside the (uncompressed) offload bundles of a host library"""
    data = open(lib, "rb").read()
    out, pos = [], data.find(MAGIC)
    while pos >= 0:
        (count,) = struct.unpack_from("<Q", data, pos + len(MAGIC))
        q = pos + len(MAGIC) + 8
        for _ in range(count):
            off, size, tlen = struct.unpack_from("<QQQ", data, q)
            triple = data[q + 24:q + 24 + tlen].decode()
            q += 24 + tlen
            if "gfx950" in triple and size:
                out.append(data[pos + off:pos + off + size])
        pos = data.find(MAGIC, pos + 1)
    if not out:
        raise SystemExit(f"{lib}: no uncompressed gfx950 code object found in its offload bundles")
    return out


def streams(lib, filters=("k_train_coop",)):
    """-> {symbol: (number of instructions, sha256 of the instruction text)} for the symbols of a library whose name contains a filter"""
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for k, img in enumerate(code_objects(lib)):
            if not any(f.encode() in img for f in filters):
                continue
            path = os.path.join(tmp, f"{k}.co")
            open(path, "wb").write(img)
            body = None
            for line in subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", path], capture_output=True, text=True, check=True).stdout.splitlines():
                m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
                if m:
                    body = res.setdefault(m.group(1), []) if any(f in m.group(1) for f in filters) else None
                elif body is not None and line.startswith("\t") and line.strip() != "...":     # ("...": objdump's elision of zero padding)
                    body.append(re.sub(r"\s+", " ", line.split("//")[0].strip()))
    return {name: (len(b), hashlib.sha256("\n".join(b).encode()).hexdigest()) for name, b in res.items() if b}


def main():
    ap = argparse.ArgumentParser(usage=__doc__)
    ap.add_argument("--filter", action="append", help="substring of the symbols to compare (default: k_train_coop)")
    ap.add_argument("before")
    ap.add_argument("after", nargs="?", default=os.path.join(ROOT, "q_learning_with_hjb_amd", "csrc", "libhjbx.so"))
    args = ap.parse_args()
    filters = tuple(args.filter or ("k_train_coop",))
    before = streams(args.before, filters)
    after = streams(args.after, filters)
    common = sorted(set(before) & set(after))
    differing = [n for n in common if before[n] != after[n]]
    missing = sorted(set(before) - set(after))
    added = sorted(set(after) - set(before))        # (e.g. the N-only epilogues of a state dimension no built-in system has)
    main_kernels = [n for n in common if re.match(r"_Z12k_train_coopI", n)]
    ok = bool(common) and not differing and not missing
    print(json.dumps(dict(tool="tools/dev/coop_isa_equal.py", compared="llvm-objdump -d per symbol, instructions without addresses and encodings",
                          **({"filters": list(filters)} if args.filter else {}), symbols_compared=len(common), k_train_coop_instantiations=len(main_kernels),
                          instructions_compared=sum(after[n][0] for n in common), identical=ok, differing=differing, missing_after=missing,
                          added_after=added), indent=1))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
