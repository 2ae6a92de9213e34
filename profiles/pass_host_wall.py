"""Wall-clock time of the five HOST forms of the query passes (rb_locate_batch, rb_hits_batch, rb_spans_batch, rb_prefix_batch,
rb_resume_batch) through the Python binding, whole call: upload, staging, the device form, copy-back.  The *_cost.py scripts report
hipEvent kernel time, which a change of the host path (allocation, copies, locks) cannot move; this one is for comparing two builds of
the library on that path (RB_AMD_LIBRARY selects the build).  README shape (four narrow filters), reads of 250 bp, every shape warmed
twice, then REPS rounds alternated over the five calls; medians, min and max.  No target.
usage: python profiles/pass_host_wall.py [--reps 9] [--reads 50000] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from readbouncer_amd import capi, synth  # noqa: E402

SEEDS = {"mock_deplete": (11, 110), "mock_t1": (12, 111), "mock_t2": (13, 112), "mock_t3": (14, 113)}
READ_LEN = 250


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--reads", type=int, default=50_000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    keys = list(SEEDS)
    built = {k: synth.build_device_filter(0, synth.WORKLOADS[k], *SEEDS[k], n_segments=512) for k in keys}
    eng = capi.Engine(0, [built[keys[0]][0]], [built[k][0] for k in keys[1:]])
    n = args.reads
    seqs, offs, lens = (t.cpu().numpy() for t in synth.make_reads_device(77, n, READ_LEN, built[keys[0]][1], torch.device("cuda:0")))
    offs, lens = offs.astype(np.uint64), lens.astype(np.uint32)
    queries = np.zeros(n, dtype=capi.SPAN_QUERY_DTYPE)
    queries["item"] = np.arange(n)
    rs = eng.resume(n, READ_LEN, READ_LEN)
    slots = np.arange(n, dtype=np.uint32)
    first = np.full(n, capi.RB_RESUME_FIRST, dtype=np.uint8)
    calls = {"locate": lambda: eng.locate(seqs, offs, lens), "hits": lambda: eng.hits(seqs, offs, lens, max_hits=8),
             "spans": lambda: eng.spans(seqs, offs, lens, 0, queries), "prefixes": lambda: eng.prefixes(seqs, offs, lens, (100, 250)),
             "resume": lambda: rs.feed(seqs, offs, lens, slots, first)}
    for fn in calls.values():
        fn(), fn()
    ms = {k: [] for k in calls}
    for _ in range(args.reps):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    lines = ["host forms, wall clock -- %s, library %s" % (torch.cuda.get_device_name(0), os.path.basename(os.environ.get("RB_AMD_LIBRARY") or capi.LIB_PATH)),
             "%d reads of %d bp, 4 filters, %d alternated repetitions" % (n, READ_LEN, args.reps)]
    lines += ["  %-8s: median %.3f ms  (min %.3f, max %.3f)" % (k, statistics.median(v), min(v), max(v)) for k, v in ms.items()]
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    rs.destroy()
    eng.destroy()


if __name__ == "__main__":
    main()
