"""What the spans pass costs: ms per 1 M queries on the located best bin, beside the locate pass on the same reads and
filters in the same run, and beside the floor of 2 h n_kmers 128-byte lines per query at the line rate that THIS run's gather probe
delivers (DeviceIBF.probe_read_peak with 128-byte rows on the same table) -- once the bin is known a k-mer costs one 8-byte word per
hash function and strand, not the whole block.  A config 3 figure below 0.8 of that floor is owed a counter run of its own.

  c3            config 3's filter (8 GiB, W = 128), 1 M reads of 360 bp, one query per read: (read, best_bin of the locate pass)
  grch38_f100k  GRCh38 at fragment_size 100 000 (W = 485), 1 M reads of 360 bp, the same
  readme        the README shape (four narrow filters), 1 M reads of 250 bp, one query per (read, filter)

Method (measuring guide): one warm-up round, then REPS alternated repetitions (locate, spans, probe, locate, spans, probe, ...), hipEvent
time of rb_engine_kernel_time, medians, the spread (min-max) stated.  A read no bin of a filter matched is asked about bin 0: the work is
the same.  usage: python profiles/spans_cost.py [--legs c3,grch38_f100k,readme] [--reps 7] [--reads 1000000] [--mask-words 0]
[--out profiles/spans/cost.txt]"""
import argparse
import os
import statistics
import sys

import numpy as np  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from readbouncer_amd import capi, synth  # noqa: E402

SEEDS = {"c3": (4, 40), "grch38_f100k": (8, 80), "mock_deplete": (11, 110), "mock_t1": (12, 111), "mock_t2": (13, 112), "mock_t3": (14, 113)}
LEGS = {"c3": (["c3"], [], 360), "readme": (["mock_deplete"], ["mock_t1", "mock_t2", "mock_t3"], 250), "grch38_f100k": (["grch38_f100k"], [], 360)}


def kernel_ms(eng, fn):
    eng.kernel_time()  # drop what is pending
    fn()
    ms, calls = eng.kernel_time()
    assert calls >= 1
    return ms


def run_leg(name, n_reads, reps, mask_words, torch, say):
    dep_keys, tgt_keys, read_len = LEGS[name]
    keys = dep_keys + tgt_keys
    built = {k: synth.build_device_filter(0, synth.WORKLOADS[k], *SEEDS[k], n_segments=512 if k.startswith("mock_") else 2048) for k in keys}
    filters = [built[k][0] for k in keys]
    nf = len(filters)
    eng = capi.Engine(0, filters[:len(dep_keys)], filters[len(dep_keys):])
    eng.set_timing(1)
    dev = torch.device("cuda:0")
    seqs, offs, lens = synth.make_reads_device(77, n_reads, read_len, built[keys[0]][1], dev)
    out = {k: torch.zeros((n_reads, nf), dtype=dt, device=dev) for k, dt in (("m", torch.int16), ("b", torch.int32), ("s", torch.uint8), ("h", torch.int32))}
    t_st = torch.zeros(n_reads, dtype=torch.uint8, device=dev)
    t_spans = torch.zeros((n_reads, 2, 6), dtype=torch.int32, device=dev)
    t_mask = torch.zeros((n_reads, 2, max(mask_words, 1)), dtype=torch.int64, device=dev)
    t_nk = torch.zeros(n_reads, dtype=torch.int32, device=dev)
    t_qs = torch.zeros(n_reads, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def locate():
        eng.locate_device(seqs.data_ptr(), offs.data_ptr(), lens.data_ptr(), n_reads, read_len, d_max_count=out["m"].data_ptr(),
                          d_best_bin=out["b"].data_ptr(), d_best_strand=out["s"].data_ptr(), d_hit_bins=out["h"].data_ptr(), d_status=t_st.data_ptr())

    locate()
    torch.cuda.synchronize()
    # the queries straight from the locate pass's output, on the device: (read, best_bin) per filter
    item = torch.arange(n_reads, dtype=torch.int32, device=dev)
    queries = [torch.stack([item, out["b"][:, fi].clamp(min=0)], dim=1).contiguous() for fi in range(nf)]
    located = int((out["b"] >= 0).sum().item())
    torch.cuda.synchronize()

    def spans():
        for fi in range(nf):
            eng.spans_device(seqs.data_ptr(), offs.data_ptr(), lens.data_ptr(), n_reads, read_len, fi, queries[fi].data_ptr(), n_reads,
                             mask_words=mask_words, d_spans=t_spans.data_ptr(), d_mask=t_mask.data_ptr() if mask_words else None,
                             d_n_kmers=t_nk.data_ptr(), d_status=t_qs.data_ptr())

    def probe():
        # G lines/s per filter: random single 128-byte rows of the filter's own table, the loads of the engine's choice
        return [f.probe_read_peak(128, int(f.info["n_words"]) * 8 > capi.nt_threshold_default(), 24, target_ms=60.0)[0] / 128.0 for f in filters]

    kernel_ms(eng, locate), kernel_ms(eng, spans), probe()  # warm-up
    loc, spn, rate = [], [], []
    for _ in range(reps):  # alternated
        loc.append(kernel_ms(eng, locate))
        spn.append(kernel_ms(eng, spans))
        rate.append(probe())
    torch.cuda.synchronize()
    assert int(t_qs.to(torch.int64).sum().item()) == 0
    pairs = n_reads * nf
    glines = [statistics.median(r[fi] for r in rate) for fi in range(nf)]
    lines = [2 * int(f.info["n_hash"]) * (read_len - int(f.info["kmer_size"]) + 1) for f in filters]  # per query
    floor_ms = sum(lines[fi] * n_reads / (glines[fi] * 1e9) * 1e3 for fi in range(nf))  # for the whole call set
    say("%s: %d reads of %d bp, %d filter(s), %d queries (%d on a located bin), mask_words %d, %d alternated repetitions" %
        (name, n_reads, read_len, nf, pairs, located, mask_words, reps))
    for label, v in (("locate", loc), ("spans", spn)):
        per_m = [x * 1e6 / pairs for x in v]
        say("  %-6s per 1 M (read, filter) pairs: median %.3f ms  (min %.3f, max %.3f)" % (label, statistics.median(per_m), min(per_m), max(per_m)))
    say("  gather probe, G lines/s per filter: %s  (min %.1f, max %.1f over the run)" %
        (", ".join("%.1f" % g for g in glines), min(min(r) for r in rate), max(max(r) for r in rate)))
    say("  lines per query: %s; floor at the probe's rate: %.3f ms per 1 M queries" % (", ".join(str(x) for x in lines), floor_ms * 1e6 / pairs))
    say("  spans / locate = %.4f;  floor / spans = %.4f" % (statistics.median(spn) / statistics.median(loc), floor_ms / statistics.median(spn)))
    eng.destroy()
    for k in built:
        built[k][0].free()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="c3,grch38_f100k,readme")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--mask-words", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spans", "cost.txt"))
    args = ap.parse_args()
    assert args.reps >= 5, "at least five alternated repetitions"
    import torch
    if capi.device_count() <= 0:
        sys.exit("spans_cost.py needs a GPU")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        def say(line):
            print(line, flush=True)
            fh.write(line + "\n")
            fh.flush()
        say("spans cost -- %s, library %s" % (torch.cuda.get_device_name(0), os.path.basename(capi.LIB_PATH)))
        for leg in args.legs.split(","):
            run_leg(leg.strip(), args.reads, args.reps, args.mask_words, torch, say)


if __name__ == "__main__":
    main()
