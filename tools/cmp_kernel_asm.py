#!/usr/bin/env python3
"""Compare two gfx950 assembly listings of one source file, kernel by kernel (mangled name).

    hipcc -std=c++17 -O3 --offload-arch=gfx950 --cuda-device-only -S file.hip -o a.s     (once per version)
    tools/cmp_kernel_asm.py old.s new.s

A kernel is `identical` when its instruction text matches with comments and blank lines stripped (the function ordinal in the
local labels .LBB<n>_<m> is dropped: it counts the kernels in front) and its VGPR / SGPR / scratch / LDS figures match.  Prints one
markdown table row per kernel that is changed, removed or added, and the totals.  Text comparison only."""
import re
import sys

FIELDS = ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size")


def kernels(path):
    """{name: (instruction text, {field: value})}"""
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)^\s*\.end_amdhsa_kernel", text, re.M | re.S):
        name, desc = m.group(1), m.group(2)
        figs = {f: re.search(r"\.amdhsa_%s\s+(\S+)" % f, desc).group(1) for f in FIELDS}
        body = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end\d+:" % re.escape(name), text, re.M | re.S).group(1)
        lines = (re.sub(r"\.LBB\d+_", ".LBB_", ln.split(";")[0]).strip() for ln in body.splitlines())
        out[name] = ("\n".join(ln for ln in lines if ln), figs)
    return out


def figures(k):
    return "%s / %s / %s / %s (%d lines)" % (*(k[1][f] for f in FIELDS), k[0].count("\n") + 1)


def main(old_path, new_path):
    old, new = kernels(old_path), kernels(new_path)
    same = [n for n in new if n in old and old[n] == new[n]]
    print("| kernel | old VGPR / SGPR / scratch / LDS | new VGPR / SGPR / scratch / LDS |")
    print("|---|---|---|")
    for n in sorted(set(old) | set(new)):
        if n not in same:
            print("| `%s` | %s | %s |" % (n, figures(old[n]) if n in old else "absent", figures(new[n]) if n in new else "removed"))
    print("\nold %d kernels, new %d: %d identical, %d changed, %d removed, %d added" % (
        len(old), len(new), len(same), len([n for n in new if n in old]) - len(same),
        len([n for n in old if n not in new]), len([n for n in new if n not in old])))


if __name__ == "__main__":
    main(*sys.argv[1:3])
