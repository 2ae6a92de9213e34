"""The compiler's resource remarks of the kernel files, for the CPU tests that pin registers, scratch, LDS and waves per SIMD at build
time (hipcc -Rpass-analysis=kernel-resource-usage, no GPU).  A unit is a translation unit of readbouncer_amd/csrc that holds kernels;
each is compiled at most once per pytest process, whichever tests ask for it."""
import atexit
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "readbouncer_amd", "csrc")
# (one today; profiles/kernel_split/README.md says what a cut by kernel family would have to keep together)
UNITS = ("rb_kernels.hip",)
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-ffp-contract=off", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage"]
REMARKS = (("occ", r"Occupancy \[waves/SIMD\]: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("vgpr", r" VGPRs: (\d+)"),
           ("lds", r"LDS Size \[bytes/block\]: (\d+)"))
_tables = {}
_tmp = None


def _demangle_args(mangled):
    """template arguments of _ZN2rb..._kernelI...EEv... as '<a,b,c>' (integers and bools only)"""
    m = re.search(r"_kernelI((?:L[ib]\d+E)+)E", mangled)
    return "<" + ",".join(re.findall(r"L[ib](\d+)E", m.group(1))) + ">" if m else ""


def parse(remarks):
    """{kernel<template arguments>: {occ, scratch, vgpr, lds}} of one compile's remarks"""
    found, cur = {}, None
    for line in remarks.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            base = re.match(r"_ZN2rb\d+(\w+?_kernel)(?=[IE]|$)", m.group(1))
            cur = (base.group(1) + _demangle_args(m.group(1))) if base else None
            if cur:
                assert cur not in found, cur
                found[cur] = {}
            continue
        if cur:
            for key, pat in REMARKS:
                m = re.search(pat, line)
                if m:
                    found[cur][key] = int(m.group(1))
    return found


def resources(unit):
    """the table of `unit` (a name of UNITS), from its one compile in this process"""
    global _tmp
    assert unit in UNITS, unit
    if unit not in _tables:
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        if not (os.path.exists(hipcc) or shutil.which(hipcc)):
            pytest.skip("no hipcc on this box: the occupancy classes are pinned where the library is built")
        if _tmp is None:
            _tmp = tempfile.mkdtemp(prefix="rb_kernel_build_")
            atexit.register(shutil.rmtree, _tmp, ignore_errors=True)
        p = subprocess.run([hipcc] + FLAGS + ["-c", os.path.join(CSRC, unit), "-o", os.path.join(_tmp, unit + ".o")],
                           capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-2000:]
        _tables[unit] = parse(p.stderr)
    return _tables[unit]


def builds(table, kernel):
    """{template arguments as a tuple of integers: resources} of one kernel's builds in a table"""
    return {tuple(int(x) for x in k[len(kernel) + 1:-1].split(",")): v for k, v in table.items() if k.startswith(kernel + "<")}
