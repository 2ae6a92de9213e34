"""What the locate pass costs: ms per 1 M located (read, filter) pairs beside the K1 time of the count kernels.

  c3            config 3's filter (8 GiB, W = 128), 1 M reads of 360 bp, ALL located, against the plain kernel with bound pruning
                switched off (rb_engine_set_bound_pruning(e, 0)) on the same filter and reads.  Expectation: parity -- the same lines in
                the same schedule plus a per-read constant; the margin is the placement-to-placement spread of tables >= 1 GiB
                (1.7-2.9 %), i.e. <= 3 % over that baseline.  The plain kernel is the same source in this build and in the
                commit before the locate pass; RB_AMD_LIBRARY=<path of that commit's library> measures its binary for the baseline.
  readme        the README shape (four narrow filters), 1 M reads of 250 bp, the reads the first pass decided on (decision != 0) located
  grch38_f100k  GRCh38 at fragment_size 100 000 (W = 485), 1 M reads of 360 bp, the same selection
                -- both beside that engine's K1 time for the WHOLE batch.  No target: it tells a user what --report-bins costs.

Method (measuring guide): one warm-up pair, then REPS alternated repetitions (K1, locate, K1, locate, ...), hipEvent kernel time of
rb_engine_kernel_time, medians, the spread (min-max) stated.  usage: python profiles/locate_cost.py [--legs c3,readme,grch38_f100k]
[--reps 7] [--reads 1000000] [--out profiles/locate/cost.txt]"""
import argparse
import os
import statistics
import sys

import numpy as np

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


def run_leg(name, n_reads, reps, torch, say):
    dep_keys, tgt_keys, read_len = LEGS[name]
    built = {k: synth.build_device_filter(0, synth.WORKLOADS[k], *SEEDS[k], n_segments=512 if k.startswith("mock_") else 2048) for k in dep_keys + tgt_keys}
    dep, tgt = [built[k][0] for k in dep_keys], [built[k][0] for k in tgt_keys]
    nf = len(dep) + len(tgt)
    eng = capi.Engine(0, dep, tgt)
    eng.set_timing(1)
    if name == "c3":
        eng.set_bound_pruning(0)
    dev = torch.device("cuda:0")
    seqs, offs, lens = synth.make_reads_device(77, n_reads, read_len, built[(dep_keys + tgt_keys)[0]][1], dev)
    t_max = torch.zeros((n_reads, nf), dtype=torch.int16, device=dev)
    t_dec = torch.zeros(n_reads, dtype=torch.uint8, device=dev)
    out = {k: torch.zeros((n_reads, nf), dtype=dt, device=dev) for k, dt in (("m", torch.int16), ("b", torch.int32), ("s", torch.uint8), ("h", torch.int32))}
    t_st = torch.zeros(n_reads, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def classify():
        eng.classify_device(seqs.data_ptr(), offs.data_ptr(), lens.data_ptr(), n_reads, read_len, d_maxcount=t_max.data_ptr(), d_decision=t_dec.data_ptr())

    classify()
    if name == "c3":
        ids, n_loc = None, n_reads
    else:
        ids = torch.nonzero(t_dec != 0).flatten().to(torch.int32).contiguous()
        n_loc = int(ids.numel())
    torch.cuda.synchronize()

    def locate():
        eng.locate_device(seqs.data_ptr(), offs.data_ptr(), lens.data_ptr(), n_loc, read_len, d_read_ids=None if ids is None else ids.data_ptr(),
                          d_max_count=out["m"].data_ptr(), d_best_bin=out["b"].data_ptr(), d_best_strand=out["s"].data_ptr(),
                          d_hit_bins=out["h"].data_ptr(), d_status=t_st.data_ptr())

    kernel_ms(eng, classify), kernel_ms(eng, locate)  # warm-up
    if ids is None:
        assert torch.equal(out["m"], t_max), "locate's maximum differs from the classify path's"
    k1, loc = [], []
    for _ in range(reps):  # alternated
        k1.append(kernel_ms(eng, classify))
        loc.append(kernel_ms(eng, locate))
    pairs = n_loc * nf
    per_m = [x * 1e6 / pairs for x in loc]
    say("%s: %d reads of %d bp, %d filter(s), %d located (%.1f %%), %d alternated repetitions" % (name, n_reads, read_len, nf, n_loc, 100.0 * n_loc / n_reads, reps))
    say("  K1 %s whole batch          : median %.3f ms  (min %.3f, max %.3f)" % ("(plain, bound pruning off)" if name == "c3" else "(engine defaults)",
                                                                                 statistics.median(k1), min(k1), max(k1)))
    say("  locate, all selected items  : median %.3f ms  (min %.3f, max %.3f)" % (statistics.median(loc), min(loc), max(loc)))
    say("  locate per 1 M (read, filter) pairs: median %.3f ms  (min %.3f, max %.3f)" % (statistics.median(per_m), min(per_m), max(per_m)))
    if name == "c3":
        ratio = statistics.median(loc) / statistics.median(k1)
        say("  locate / K1 = %.4f  (expectation: <= 1.03, the placement-to-placement spread of tables >= 1 GiB)" % ratio)
    eng.destroy()
    for k in built:
        built[k][0].free()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="c3,readme,grch38_f100k")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "locate", "cost.txt"))
    args = ap.parse_args()
    assert args.reps >= 5, "at least five alternated repetitions"
    import torch
    if capi.device_count() <= 0:
        sys.exit("locate_cost.py needs a GPU")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        def say(line):
            print(line, flush=True)
            fh.write(line + "\n")
            fh.flush()
        say("locate cost -- %s, library %s" % (torch.cuda.get_device_name(0), os.path.basename(capi.LIB_PATH)))
        for leg in args.legs.split(","):
            run_leg(leg.strip(), args.reads, args.reps, torch, say)


if __name__ == "__main__":
    main()
