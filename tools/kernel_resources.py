#!/usr/bin/env python3
"""Table of the compiler's resource report (hipcc -Rpass-analysis=kernel-resource-usage, stderr) for the kernels whose demangled name
starts with a prefix: VGPRs, AGPRs, SGPRs, scratch, spills, waves per SIMD.  Usage: kernel_resources.py LOG [PREFIX ...]"""
import re
import subprocess
import sys


def parse(path):
    rows, cur = [], None
    for line in open(path):
        m = re.search(r"remark:\s+(Function Name|[A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+)", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = {"name": val}
            rows.append(cur)
        elif cur is not None:
            cur[key] = val
    names = subprocess.run(["c++filt"], input="\n".join(r["name"] for r in rows), capture_output=True, text=True).stdout.split("\n")
    for r, n in zip(rows, names):
        r["name"] = re.sub(r"\(.*", "", n).replace("void ", "")
    return rows


def main():
    rows = parse(sys.argv[1])
    prefixes = sys.argv[2:]
    print(f"{'kernel':60s} {'VGPR':>5s} {'AGPR':>5s} {'SGPR':>5s} {'scratch':>7s} {'spill':>5s} {'waves':>5s}")
    for r in sorted(rows, key=lambda r: r["name"]):
        if prefixes and not any(p in r["name"] for p in prefixes):
            continue
        spill = int(r.get("SGPRs Spill", 0)) + int(r.get("VGPRs Spill", 0))
        print(f"{r['name']:60s} {r.get('VGPRs', '?'):>5s} {r.get('AGPRs', '?'):>5s} {r.get('TotalSGPRs', '?'):>5s} {r.get('ScratchSize', '?'):>7s} {spill:>5d} {r.get('Occupancy', '?'):>5s}")


if __name__ == "__main__":
    main()
