#!/usr/bin/env python3
"""Are the kernels of two trees the same?  Compares gfx950 device assembly per kernel after stripping comments, directives, labels and symbol names.

    for u in ahc_startup ahc_rounds ahc_batch ahc_ro ahc_rom; do      (in each tree's fluidaudio_amd/csrc, with the units' Makefile flags)
        hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -mllvm -amdgpu-kernarg-preload-count=14 --cuda-device-only -S $u.hip -o DIR/$u.s
    done
    kernel_compare.py PARENT_DIR BRANCH_DIR
"""
import glob
import os
import re
import subprocess
import sys


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return dict(zip(names, out)) if len(out) == len(names) else {n: n for n in names}


def kernels(path):
    text = open(path).read()
    found = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M):
        name = m.group(1)
        i = text.index("\n" + name + ":")
        j = text.index(".Lfunc_end", i)
        body = []
        for line in text[i:j].split("\n")[1:]:
            t = line.split(";")[0].strip()
            if not t or t.startswith(".") or re.match(r"^[.A-Za-z_0-9$]+:$", t):
                continue
            t = re.sub(r"\.L[A-Za-z_0-9$]+", "L", t)                 # branch targets
            t = re.sub(r"\b_Z[A-Za-z_0-9$.]+", "SYM", t)            # symbol names
            body.append(t)
        k = text.index(".amdhsa_kernel " + name)
        desc = text[k:text.index(".end_amdhsa_kernel", k)]
        res = {key: (re.search(r"\.amdhsa_" + key + r"\s+(\S+)", desc) or [None, "?"])[1]
               for key in ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size")}
        found[name] = (body, res)
    return found


def main():
    parent, branch = sys.argv[1], sys.argv[2]
    units = sorted(os.path.basename(p) for p in glob.glob(os.path.join(parent, "*.s")))
    same = total = 0
    rows = []
    for u in units:
        a, b = kernels(os.path.join(parent, u)), kernels(os.path.join(branch, u))
        names = demangle(sorted(set(a) | set(b)))
        if set(a) != set(b):
            rows.append(f"{u}: DIFFERENT kernel sets: only parent {sorted(set(a) - set(b))}, only branch {sorted(set(b) - set(a))}")
        for n in sorted(set(a) & set(b), key=lambda n: names[n].replace('(anonymous namespace)::', '')):
            total += 1
            ident = a[n][0] == b[n][0] and a[n][1] == b[n][1]
            same += ident
            r = a[n][1]
            rows.append(f"{names[n].replace('(anonymous namespace)::', '').replace('void ', '').split('(')[0]} ({u[:-2]}.hip): parent {len(a[n][0])} instr | branch {len(b[n][0])} instr | {'IDENTICAL' if ident else 'DIFFERENT'} | "
                        f"VGPR {r['next_free_vgpr']} SGPR {r['next_free_sgpr']} LDS {r['group_segment_fixed_size']} scratch {r['private_segment_fixed_size']}"
                        + (" | same" if a[n][1] == b[n][1] else f" | branch {b[n][1]}"))
    print(f"{same} of {total} kernels instruction-identical")
    print("\n".join(rows))


if __name__ == "__main__":
    main()
