"""The kernel translation units together hold every kernel build exactly once (hipcc, no GPU; the compiles of tests/kernel_build.py).
A kernel template is instantiated by the launchers that name it, so a launcher that goes, or moves to another unit without its kernel,
or a family compiled into two units, changes the set of builds without any error at build time: the first two drop builds from the
library, the third registers one kernel from two code objects.  The counts are those of the device listing of rb_kernels.hip."""
from collections import Counter

from tests.kernel_build import UNITS, resources

# kernel -> builds (template instantiations) in the library
BUILDS = {
    "ibf_count_max_kernel": 64, "ibf_count_max_split_kernel": 32, "ibf_hits_kernel": 30, "ibf_locate_kernel": 30, "ibf_prefix_kernel": 30,
    "ibf_resume_kernel": 20, "ibf_count_max_merged_kernel": 16, "ibf_count_rows_kernel": 16, "ibf_count_max_phased_kernel": 14,
    "ibf_count_max_phased_multi_kernel": 12, "ibf_bin_occupancy_kernel": 4, "ibf_count_max_split_any_kernel": 4, "ibf_spans_kernel": 4,
    "ibf_assemble_kernel": 2,
    # the kernels that are no templates
    "chunk_prep_kernel": 1, "compare_bits_kernel": 1, "copy_from_host_kernel": 1, "decide_kernel": 1, "fill_reads_kernel": 1,
    "fill_synth_kernel": 1, "finish_hits_kernel": 1, "finish_prefix_kernel": 1, "first_decided_kernel": 1, "ibf_insert_kernel": 1,
    "ibf_row_table_kernel": 1, "invert_words_kernel": 1, "merge_bits_kernel": 1, "reduce_locate_slices_kernel": 1, "reduce_slices_kernel": 1,
    "restride_blocks_kernel": 1, "resume_commit_kernel": 1, "resume_counts_kernel": 1, "resume_prep_kernel": 1,
}


def test_every_kernel_build_is_in_exactly_one_unit():
    assert sum(BUILDS.values()) == 297 and sum(1 for n in BUILDS.values() if n == 1) == 19
    where = {}
    for unit in UNITS:
        for build in resources(unit):
            where.setdefault(build, []).append(unit)
    twice = {b: u for b, u in where.items() if len(u) > 1}
    assert not twice, twice
    got = Counter(b.split("<")[0] for b in where)
    assert dict(got) == BUILDS, sorted(set(got.items()) ^ set(BUILDS.items()))
    # a family is whole: all builds of a kernel come from one unit
    split = {k for k in BUILDS if len({where[b][0] for b in where if b.split("<")[0] == k}) != 1}
    assert not split, split
