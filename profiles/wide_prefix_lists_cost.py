#!/usr/bin/env python3
"""The wide list form of the prefix pass (rb_engine_set_wide_prefix_lists: ibf_prefix_wide_lists_kernel on the filter's wide list table)
on the filter of bench leg grch38_f100k (synth.WORKLOADS: GRCh38 at fragment_size 100 000, about 31 000 bins, W = 485, built once with
bench.py's seeds): reads of 1 440 bp, checkpoints 360 / 720 / 1 080 / 1 440 -- the shape of profiles/prefix/cost.txt.  One process, one
warm-up round, then alternated rounds of
  (a)  the prefix pass under RB_PASS_LISTS_OFF
  (a') the prefix pass under RB_PASS_LISTS_CURRENT (rb_engine_wide_prefix_lines and the item counters are printed)
  (b') the wide locate pass over the whole reads (rb_engine_set_wide_pass_lists)
  (c') the four chunked classify calls with rb_engine_set_wide_lists on, as the engine runs them
hipEvent kernel time of rb_engine_kernel_time (for a pass every kernel of the call; (c') summed over its four calls), median of the
repeats with min and max.  Reports (a)/(a'), (a')/(b'), (a')/(c') and checks that every output of the prefix pass is byte-identical
between OFF and CURRENT, that its maxima and decisions are the chunked calls' and its last checkpoint's maxima the locate pass's.

  python3 profiles/wide_prefix_lists_cost.py [reads, default 250000] [repeats, default 5] [--out FILE]
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from readbouncer_amd import capi, synth  # noqa: E402

argv = sys.argv[1:]
out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
args = [a for i, a in enumerate(argv) if a != "--out" and (i == 0 or argv[i - 1] != "--out")]
n = int(args[0]) if len(args) > 0 else 250_000
reps = int(args[1]) if len(args) > 1 else 5
READ_LEN, CHECKPOINTS = 1440, (360, 720, 1080, 1440)
P = len(CHECKPOINTS)
OFF, CURRENT = capi.RB_PASS_LISTS_OFF, capi.RB_PASS_LISTS_CURRENT
lines_out = []


def say(*parts):
    line = " ".join(str(p) for p in parts)
    print(line, flush=True)
    lines_out.append(line)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write("\n".join(lines_out) + "\n")


dev = torch.device("cuda:0")
d, ref = synth.build_device_filter(0, synth.WORKLOADS["grch38_f100k"], fill_seed=8, plant_seed=80)
torch.cuda.synchronize()
eng = capi.Engine(0, [d], [])
eng.set_split_threshold(0)
eng.set_timing(1)
say("filter", json.dumps({k: int(v) for k, v in d.info.items()}))
info = d.wide_list_table_build()
say("table", json.dumps({k: info[k] for k in ("bytes", "rows", "lines", "side_rows", "refused")}))
assert info["refused"] == 0 and info["lines"] in (4, 6, 8)
eng.set_wide_lists(CURRENT)
eng.set_wide_pass_lists(CURRENT)
seqs, offs, lens = synth.make_reads_device(77, n, READ_LEN, ref, dev)
p = {s: {"max": torch.zeros((n, P, 1), dtype=torch.int16, device=dev), "dec": torch.zeros((n, P), dtype=torch.uint8, device=dev),
         "best": torch.zeros((n, P), dtype=torch.int32, device=dev), "st": torch.zeros((n, P), dtype=torch.uint8, device=dev),
         "len": torch.zeros((n, P), dtype=torch.int32, device=dev), "first": torch.zeros(n, dtype=torch.int32, device=dev)} for s in (OFF, CURRENT)}
c_max = torch.zeros((P, n, 1), dtype=torch.int16, device=dev)
c_dec = torch.zeros((P, n), dtype=torch.uint8, device=dev)
loc = {k: torch.zeros((n, 1), dtype=dt, device=dev) for k, dt in (("m", torch.int16), ("b", torch.int32), ("s", torch.uint8), ("h", torch.int32))}
l_st = torch.zeros(n, dtype=torch.uint8, device=dev)
torch.cuda.synchronize()


def prefixes(setting):
    def go():
        eng.set_wide_prefix_lists(setting)
        assert eng.wide_prefix_lines(0, READ_LEN, CHECKPOINTS[-1]) == (info["lines"] if setting == CURRENT else 0)
        o = p[setting]
        eng.prefixes_device(seqs.data_ptr(), offs.data_ptr(), lens.data_ptr(), n, READ_LEN, CHECKPOINTS, d_max_count=o["max"].data_ptr(),
                            d_decision=o["dec"].data_ptr(), d_best_target=o["best"].data_ptr(), d_status=o["st"].data_ptr(),
                            d_prefix_len=o["len"].data_ptr(), d_first_decided=o["first"].data_ptr())
    return go


def locate():
    eng.locate_device(seqs.data_ptr(), offs.data_ptr(), lens.data_ptr(), n, READ_LEN, d_max_count=loc["m"].data_ptr(),
                      d_best_bin=loc["b"].data_ptr(), d_best_strand=loc["s"].data_ptr(), d_hit_bins=loc["h"].data_ptr(), d_status=l_st.data_ptr())


def chunked():
    for i, c in enumerate(CHECKPOINTS):
        eng.classify_device_ex(seqs.data_ptr(), offs.data_ptr(), lens.data_ptr(), n, READ_LEN, chunk_length=c, d_maxcount=c_max[i].data_ptr(),
                               d_decision=c_dec[i].data_ptr())


def kernel_ms(fn):
    torch.cuda.synchronize()
    eng.kernel_time()  # drop what is pending
    fn()
    torch.cuda.synchronize()
    ms, calls = eng.kernel_time()
    assert calls >= 1
    return ms


legs = (("a_off", prefixes(OFF)), ("a_current", prefixes(CURRENT)), ("b_wide_locate", locate), ("c_wide_chunked", chunked))
say("plan classify", eng.plan(0, n, READ_LEN)["kernel"], "; wide_pass_lines", eng.wide_pass_lines(0, READ_LEN))
eng.wide_prefix_lists_items(reset=True)
for _, fn in legs:  # warm-up
    kernel_ms(fn)
say("items taken / left by the wide form in one call:", eng.wide_prefix_lists_items())
same = all(torch.equal(p[OFF][k], p[CURRENT][k]) for k in p[OFF])
say("prefix outputs byte-identical between OFF and CURRENT:", same)
assert same
assert torch.equal(p[CURRENT]["max"].permute(1, 0, 2), c_max) and torch.equal(p[CURRENT]["dec"].permute(1, 0), c_dec), "prefix pass != chunked classify"
assert torch.equal(p[CURRENT]["max"][:, P - 1, :], loc["m"]), "the last checkpoint's maxima differ from the locate pass's"
ms = {key: [] for key, _ in legs}
for rep in range(reps):  # alternated
    for key, fn in (legs[::-1] if rep % 2 else legs):
        ms[key].append(kernel_ms(fn))
med = {key: statistics.median(v) for key, v in ms.items()}
say("%d reads of %d bp, checkpoints %s, %d alternated repetitions" % (n, READ_LEN, "/".join(map(str, CHECKPOINTS)), reps))
for key, _ in legs:
    say("  %-15s median %.3f ms  (min %.3f, max %.3f, spread %.2f %%)" % (key, med[key], min(ms[key]), max(ms[key]),
                                                                       100.0 * (max(ms[key]) - min(ms[key])) / med[key]))
say("  off / current = %.3f   current / wide locate = %.4f   current / wide chunked classify = %.4f" %
    (med["a_off"] / med["a_current"], med["a_current"] / med["b_wide_locate"], med["a_current"] / med["c_wide_chunked"]))
assert all(torch.equal(p[OFF][k], p[CURRENT][k]) for k in p[OFF])
eng.destroy()
