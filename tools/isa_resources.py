#!/usr/bin/env python
"""Kernel resources from the gfx950 ISA hipcc emits (no GPU needed): registers, scratch, LDS, occupancy, code length, the instruction count
and the counts of MFMA, s_nop and branch instructions of every kernel of the given csrc/*.hip files, for this tree or for another checkout of it.
LFDM_ISA_FLAGS in the environment adds compiler flags (a probe build's -D switch).

    tools/isa_resources.py scan OUT.json [--root DIR] file.hip ...     DIR: the checkout whose cvpr23_lfdm_amd/csrc holds the files (default: this tree)
    tools/isa_resources.py table PARENT.json TREE.json                 one line per kernel, 'a->b' where the two differ (the format of
                                                                       profiles/conv_core_refactor_ab.txt section 1), 'identical' where the
                                                                       kernel body disassembles identically (comments and label numbers
                                                                       aside), and the condition line; exit status 1 when the condition
                                                                       is False (a kernel gained scratch, lost a wave of occupancy or
                                                                       changed its LDS size)"""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-mllvm", "-amdgpu-mfma-vgpr-form", "-S", "--cuda-device-only"]
FIELDS = ["VGPRs", "scratch", "LDS", "occ", "codeLen", "insts", "MFMA", "s_nop", "branch"]


def demangle(name):
    out = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip() or name
    out = re.sub(r"^void ", "", out).replace("(anonymous namespace)::", "")
    return re.sub(r"\(.*$", "", out)


def scan(root, files):
    res = {}
    for f in files:
        src = os.path.join(root, "cvpr23_lfdm_amd", "csrc", os.path.basename(f))
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, "k.s")
            r = subprocess.run([HIPCC] + FLAGS + os.environ.get("LFDM_ISA_FLAGS", "").split() + ["-o", out, src], capture_output=True, text=True)
            if r.returncode != 0:
                sys.exit("%s: hipcc failed\n%s" % (src, r.stderr[-2000:]))
            text = open(out).read()
        for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?\n; Occupancy: \d+)", text, re.S | re.M):
            name, body = m.group(1), m.group(2)
            insts = [l.strip() for l in body.split("\n") if l.startswith("\t") and not l.strip().startswith((";", "."))]

            def note(key):
                mm = re.search(r"; %s(?::| =) (\d+)" % key, body)
                return int(mm.group(1)) if mm else -1
            res["%s %s" % (os.path.basename(f)[:-4], demangle(name))] = {
                "VGPRs": note("NumVgprs") if note("TotalNumVgprs") < 0 else note("TotalNumVgprs"), "scratch": note("ScratchSize"),
                "LDS": note("LDSByteSize"), "occ": note(r"Occupancy"), "codeLen": note("codeLenInByte"), "insts": len(insts),
                "MFMA": sum(i.startswith("v_mfma") for i in insts), "s_nop": sum(i.startswith("s_nop") for i in insts),
                "branch": sum(i.startswith(("s_cbranch", "s_branch")) for i in insts),
                # the kernel body, comments and label numbers aside: equal hashes = 'identical' in the table
                "isa": hashlib.sha256("\n".join(re.sub(r"\.LBB\d+_\d+", ".LBB", re.sub(r"\s*;.*$", "", i)) for i in insts).encode()).hexdigest()[:16]}
    return res


def table(pa, tr):
    A, B = json.load(open(pa)), json.load(open(tr))
    bad = lds = 0
    print("%-16s %-58s " % ("file", "kernel") + " ".join("%-14s" % f for f in FIELDS) + " ISA vs parent")
    # a kernel that gained a trailing bool template argument is set against the parent's kernel without it
    parent_of = {k: k if k in A else re.sub(r", (true|false)>$", ">", k) for k in B}
    for k in sorted(set(B) | (set(A) - set(parent_of.values()))):
        a, b = A.get(parent_of.get(k, k)), B.get(k)
        f, kern = k.split(" ", 1)
        cells = []
        for fld in FIELDS:
            x, y = (a or {}).get(fld, "-"), (b or {}).get(fld, "-")
            cells.append("%-14s" % (x if x == y else "%s->%s" % (x, y)))
        if a and b and "isa" in a and "isa" in b:
            cells.append("identical" if a["isa"] == b["isa"] else "differs  ")
        if a and b and (b["scratch"] > a["scratch"] or b["occ"] < a["occ"]):
            bad += 1
            cells.append("WORSE")
        if a and b and b["LDS"] != a["LDS"]:
            lds += 1
        print("%-16s %-58s " % (f, kern) + " ".join(cells))
    print("# %d kernels, %d gained scratch or lost occupancy, %d with another LDS size" % (len(B), bad, lds))
    print("condition (no kernel gains scratch, none loses a wave of occupancy, LDS equal everywhere): %s" % (bad == 0 and lds == 0))
    return 1 if bad or lds else 0


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "scan":
        args = sys.argv[3:]
        root = ROOT
        if args[0] == "--root":
            root, args = os.path.abspath(args[1]), args[2:]
        json.dump(scan(root, args), open(sys.argv[2], "w"), indent=1, sort_keys=True)
    elif len(sys.argv) == 4 and sys.argv[1] == "table":
        sys.exit(table(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
