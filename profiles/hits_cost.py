"""What the hits pass costs: ms per 1 M (read, filter) pairs beside the locate pass on the same reads and filter in the
same run -- the gathers are the same, and at the decision threshold hits are rare, so the expectation is parity within the
placement-to-placement spread of large tables (about 3 %).  A ratio outside it is owed a rocprofv3 --kernel-trace --stats run.

  c3            config 3's filter (8 GiB, W = 128), 1 M reads of 360 bp, all of them, min_count = 0, max_hits = 8
  grch38_f100k  GRCh38 at fragment_size 100 000 (W = 485), 1 M reads of 360 bp, the same
  readme        the README shape (four narrow filters), 1 M reads of 250 bp, the same
  dense         the README shape's deplete filter alone, min_count = 1, max_hits = 2 x n_bins on --dense-reads reads: every k-mer
                that is in any bin makes a record.  Stated, not gated.

Method (measuring guide): one warm-up pair, then REPS alternated repetitions (locate, hits, locate, hits, ...), hipEvent time of
rb_engine_kernel_time, medians, the spread (min-max) stated.  usage: python profiles/hits_cost.py [--legs c3,grch38_f100k,readme,dense]
[--reps 7] [--reads 1000000] [--dense-reads 100000] [--out profiles/hits/cost.txt]"""
import argparse
import os
import statistics
import sys

import numpy as np  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from readbouncer_amd import capi, synth  # noqa: E402

SEEDS = {"c3": (4, 40), "grch38_f100k": (8, 80), "mock_deplete": (11, 110), "mock_t1": (12, 111), "mock_t2": (13, 112), "mock_t3": (14, 113)}
LEGS = {"c3": (["c3"], [], 360), "readme": (["mock_deplete"], ["mock_t1", "mock_t2", "mock_t3"], 250), "grch38_f100k": (["grch38_f100k"], [], 360),
        "dense": (["mock_deplete"], [], 250)}


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
    dev = torch.device("cuda:0")
    seqs, offs, lens = synth.make_reads_device(77, n_reads, read_len, built[(dep_keys + tgt_keys)[0]][1], dev)
    dense = name == "dense"
    n_bins = sum(int(d.info["n_bins"]) for d in dep + tgt)
    cap = 2 * n_bins if dense else 8
    min_count = 1 if dense else 0
    out = {k: torch.zeros((n_reads, nf), dtype=dt, device=dev) for k, dt in (("m", torch.int16), ("b", torch.int32), ("s", torch.uint8), ("h", torch.int32))}
    t_hits = torch.zeros((n_reads, nf, cap, 2), dtype=torch.int32, device=dev)
    t_n = torch.zeros((n_reads, nf), dtype=torch.int32, device=dev)
    t_bins = torch.zeros(n_bins, dtype=torch.int64, device=dev)
    t_st = torch.zeros(n_reads, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def locate():
        eng.locate_device(seqs.data_ptr(), offs.data_ptr(), lens.data_ptr(), n_reads, read_len, d_max_count=out["m"].data_ptr(),
                          d_best_bin=out["b"].data_ptr(), d_best_strand=out["s"].data_ptr(), d_hit_bins=out["h"].data_ptr(), d_status=t_st.data_ptr())

    def hits():
        eng.hits_device(seqs.data_ptr(), offs.data_ptr(), lens.data_ptr(), n_reads, read_len, min_count=min_count, max_hits=cap,
                        d_hits=t_hits.data_ptr(), d_n_hits=t_n.data_ptr(), d_status=t_st.data_ptr(), d_bin_reads=t_bins.data_ptr())

    kernel_ms(eng, locate), kernel_ms(eng, hits)  # warm-up
    loc, hit = [], []
    for _ in range(reps):  # alternated
        loc.append(kernel_ms(eng, locate))
        hit.append(kernel_ms(eng, hits))
    torch.cuda.synchronize()
    pairs = n_reads * nf
    records = int(t_n.to(torch.int64).sum().item())
    say("%s: %d reads of %d bp, %d filter(s), min_count %d, max_hits %d, %d alternated repetitions; %.3f records per (read, filter) pair" %
        (name, n_reads, read_len, nf, min_count, cap, reps, records / pairs))
    for label, v in (("locate", loc), ("hits", hit)):
        per_m = [x * 1e6 / pairs for x in v]
        say("  %-6s per 1 M (read, filter) pairs: median %.3f ms  (min %.3f, max %.3f)" % (label, statistics.median(per_m), min(per_m), max(per_m)))
    say("  hits / locate = %.4f" % (statistics.median(hit) / statistics.median(loc)))
    eng.destroy()
    for k in built:
        built[k][0].free()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="c3,grch38_f100k,readme,dense")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--dense-reads", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hits", "cost.txt"))
    args = ap.parse_args()
    assert args.reps >= 5, "at least five alternated repetitions"
    import torch
    if capi.device_count() <= 0:
        sys.exit("hits_cost.py needs a GPU")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        def say(line):
            print(line, flush=True)
            fh.write(line + "\n")
            fh.flush()
        say("hits cost -- %s, library %s" % (torch.cuda.get_device_name(0), os.path.basename(capi.LIB_PATH)))
        for leg in args.legs.split(","):
            leg = leg.strip()
            run_leg(leg, args.dense_reads if leg == "dense" else args.reads, args.reps, torch, say)


if __name__ == "__main__":
    main()
