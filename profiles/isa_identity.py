#!/usr/bin/env python3
"""Which kernels of rb_kernels.hip have the same code in two builds?  Takes two device assembly listings of the file
(hipcc -O3 -std=c++17 -fPIC -fvisibility=hidden -ffp-contract=off --offload-arch=gfx950 --cuda-device-only -S), splits each per kernel
and compares, kernel by kernel, the instruction lines and the .amdhsa_ resource block.  Comments and the function number inside local
labels (.LBB<n>_<m>) are not code: they change when another function comes or goes.  Kernels named in --changed are expected to differ
and are only listed.  Usage: python3 profiles/isa_identity.py before.s after.s --changed ibf_locate_kernel ibf_hits_kernel ..."""
import argparse
import re
import subprocess


def kernels(path):
    """mangled name -> (instruction lines, .amdhsa_ lines)"""
    text, hsa, cur, block = {}, {}, None, None
    for raw in open(path):
        line = raw.split(";", 1)[0].rstrip()
        line = re.sub(r"\.L(BB|func_end|func_begin|tmp)\d+", r".L\1", line)
        s = line.strip()
        if not s:
            continue
        m = re.match(r"\.amdhsa_kernel\s+(\S+)", s)
        if m:
            block = hsa.setdefault(m.group(1), [])
            continue
        if s == ".end_amdhsa_kernel":
            block = None
            continue
        if block is not None:
            block.append(s)
            continue
        m = re.match(r"\.type\s+(\S+),@function", s)
        if m:
            cur = text.setdefault(m.group(1), [])
            continue
        if s.startswith(".Lfunc_end"):
            cur = None
            continue
        if cur is not None and not re.match(r"\.(p2align|globl|protected|weak|hidden|section|text)\b", s):
            cur.append(s)
    return {k: (text.get(k, []), hsa[k]) for k in hsa}


def base_names(mangled):
    """mangled names -> the kernels' plain names, one c++filt call for all"""
    out = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True).stdout.splitlines()
    return {m: re.sub(r"^void\s+", "", d).split("<")[0].split("(")[0].replace("rb::", "") for m, d in zip(mangled, out)}


ap = argparse.ArgumentParser()
ap.add_argument("before")
ap.add_argument("after")
ap.add_argument("--changed", nargs="*", default=[])
a = ap.parse_args()
old, new = kernels(a.before), kernels(a.after)
only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
both = sorted(set(old) & set(new))
name = base_names(both)
pinned = [k for k in both if name[k] not in a.changed]
free = [k for k in both if name[k] in a.changed]
differ = [k for k in pinned if old[k] != new[k]]
print("kernels before / after: %d / %d; only before: %d; only after: %d" % (len(old), len(new), len(only_old), len(only_new)))
for k in only_old + only_new:
    print("  not in both: %s" % k)
print("kernels that must not change: compared %d, identical %d, different %d" % (len(pinned), len(pinned) - len(differ), len(differ)))
for k in differ:
    print("  DIFFERENT: %s (%d -> %d instruction lines)" % (k, len(old[k][0]), len(new[k][0])))
same_free = sum(old[k] == new[k] for k in free)
print("kernels this change rewrites (%s): %d builds, %d of them identical all the same" % (", ".join(a.changed), len(free), same_free))
raise SystemExit(1 if differ or only_old or only_new else 0)
