"""LDS of the plain count kernel's builds, checked at build time on a CPU (hipcc -Rpass-analysis=kernel-resource-usage, no GPU; the
compile of test_kernel_resources.py).  The builds that lead with the stronger strand (rb_kernels.hip, ibf_count_max_kernel: LG == 6,
H > 0, no early decision) park a strand's probe counters in LDS -- 7 planes x words per lane x 64 lanes x 8 bytes per wave, 28 KiB per
workgroup on the two-word builds.  They are compiled for three waves per SIMD = three workgroups of four waves per CU, so three
workgroups' LDS must fit the CU's 160 KiB, or the LDS and not the registers would set the occupancy without any compiler report saying
so.  The H = 3 builds must also keep their waves per SIMD and stay free of scratch."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "readbouncer_amd", "csrc")
CU_LDS_BYTES = 160 * 1024
WORKGROUPS_PER_CU = 3  # 3 waves per SIMD x 4 SIMDs / 4 waves per workgroup

# <LG, words per lane, planes, H, NT, EARLY> of the builds with H = 3 that take the bound -> least waves per SIMD
OCCUPANCY = {(6, 2, 10, 3): 3, (6, 2, 16, 3): 3, (6, 1, 10, 3): 4, (6, 1, 16, 3): 4}


def _args(mangled):
    m = re.search(r"_kernelI((?:L[ib]\d+E)+)E", mangled)
    return tuple(int(x) for x in re.findall(r"L[ib](\d+)E", m.group(1))) if m else ()


@pytest.fixture(scope="module")
def plain_builds(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc on this box: the resource classes are pinned where the library is built")
    out = tmp_path_factory.mktemp("lds") / "k.o"
    p = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-ffp-contract=off", "--offload-arch=gfx950",
                        "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "rb_kernels.hip"), "-o", str(out)],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    found, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = _args(m.group(1)) if re.search(r"\d+ibf_count_max_kernelI", m.group(1)) else None
            if cur:
                found[cur] = {}
            continue
        if cur:
            for key, pat in (("occ", r"Occupancy \[waves/SIMD\]: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                             ("lds", r"LDS Size \[bytes/block\]: (\d+)"), ("vgpr", r" VGPRs: (\d+)")):
                m = re.search(pat, line)
                if m:
                    found[cur][key] = int(m.group(1))
    assert len(found) >= 20, sorted(found)
    return found


def test_three_workgroups_of_lds_fit_a_cu(plain_builds):
    over = {k: v for k, v in plain_builds.items() if v["lds"] * WORKGROUPS_PER_CU > CU_LDS_BYTES}
    assert not over, over
    # the builds that lead hold the parked planes; the others (early-decision twins, narrow blocks, run-time hashes) only the staged bases
    for (lg, wpl, np_, h, nt, early), v in plain_builds.items():
        leads = lg == 6 and h > 0 and not early
        want = 4 * 7 * wpl * 64 * 8 if leads else 0
        assert want <= v["lds"] < want + 4096, ((lg, wpl, np_, h, nt, early), v)


def test_h3_builds_keep_occupancy_and_no_scratch(plain_builds):
    seen = 0
    for (lg, wpl, np_, h, nt, early), v in plain_builds.items():
        if (lg, wpl, np_, h) in OCCUPANCY:
            seen += 1
            assert v["occ"] >= OCCUPANCY[(lg, wpl, np_, h)] and v["scratch"] == 0, ((lg, wpl, np_, h, nt, early), v)
    assert seen >= 2 * len(OCCUPANCY), seen  # (both table policies of every build)
