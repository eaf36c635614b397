"""Register and segment figures of the ten wave-per-value circuit kernels (kernels.hip), from the
compiler's own metadata: kernels.hip is compiled for gfx950 to assembly (device only, no GPU
needed) and the VGPRs, SGPRs, private segment, spill counts and kernarg size of gate, borrow,
minmax, select, lookup, shift, bitcount, bitrun, array_read and array_write are read from it; tools/kernarg_audit.py's findings are counted
beside them.

usage: circuit_resources.py [--src homomorph-rust_amd/csrc/kernels.hip] [--label new]
                            [--out profiles/circuits/resources.json]
The output file maps labels to tables; an existing file keeps its other labels.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernarg_audit  # noqa: E402

KERNELS = ("gate", "borrow", "minmax", "select", "lookup", "shift", "bitcount", "bitrun",
           "array_read", "array_write")
FIELDS = {"vgpr_count": "vgprs", "sgpr_count": "sgprs", "private_segment_fixed_size": "private",
          "vgpr_spill_count": "vgpr_spills", "sgpr_spill_count": "sgpr_spills",
          "kernarg_segment_size": "kernarg_bytes"}


def resources(src):
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "kernels.s")
        subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950",
                        "-Wno-unused-result", "--cuda-device-only", "-S", src, "-o", asm], check=True)
        text = open(asm).read()
        audit = kernarg_audit.parse(asm)
    table = {}
    for block in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        short = re.match(r"_ZN2hm\d+(\w+?)_kernelENS", name)
        if not short or short.group(1) not in KERNELS:
            continue
        row = {v: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1)) for k, v in FIELDS.items()}
        row["kernarg_audit_findings"] = len(audit[name]["findings"])
        table[short.group(1)] = row
    assert sorted(table) == sorted(KERNELS), sorted(table)
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", default=os.path.join(ROOT, "homomorph-rust_amd", "csrc", "kernels.hip"))
    ap.add_argument("--label", default="new")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "circuits", "resources.json"))
    args = ap.parse_args()
    doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
    doc[args.label] = resources(args.src)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc[args.label], indent=1))


if __name__ == "__main__":
    main()
