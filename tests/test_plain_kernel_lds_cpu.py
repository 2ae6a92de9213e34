"""LDS of the plain count kernel's builds, checked at build time on a CPU (hipcc -Rpass-analysis=kernel-resource-usage, no GPU; the
compile of test_kernel_resources.py).  The builds that lead with the stronger strand (rb_kernels.hip, ibf_count_max_kernel: LG == 6,
H > 0, no early decision) park a strand's probe counters in LDS -- 7 planes x words per lane x 64 lanes x 8 bytes per wave, 28 KiB per
workgroup on the two-word builds.  They are compiled for three waves per SIMD = three workgroups of four waves per CU, so three
workgroups' LDS must fit the CU's 160 KiB, or the LDS and not the registers would set the occupancy without any compiler report saying
so.  The H = 3 builds must also keep their waves per SIMD and stay free of scratch."""
import pytest

from tests.kernel_build import builds, resources

CU_LDS_BYTES = 160 * 1024
WORKGROUPS_PER_CU = 3  # 3 waves per SIMD x 4 SIMDs / 4 waves per workgroup

# <LG, words per lane, planes, H, NT, EARLY> of the builds with H = 3 that take the bound -> least waves per SIMD
OCCUPANCY = {(6, 2, 10, 3): 3, (6, 2, 16, 3): 3, (6, 1, 10, 3): 4, (6, 1, 16, 3): 4}


@pytest.fixture(scope="module")
def plain_builds():
    found = builds(resources("rb_kernels.hip"), "ibf_count_max_kernel")
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
