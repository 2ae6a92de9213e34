"""What resumable counting costs: a read of 1 440 bp fed in four chunks of 360 bp onto a slot in HBM, beside what the
same four decisions cost today.

  c3      config 3's filter (8 GiB, W = 128): a slot holds 2 x 16 x 128 words = 32 KiB
  readme  the README shape (four narrow filters)
both with one slot per read, all reads, in ONE process:
  (r) the four feeds (rb_resume_batch_device with chunk_start = 0 / 360 / 720 / 1 080, chunk_length = 360; every output asked for)
  (c) the four rb_classify_batch_device_ex calls on the prefixes 360 / 720 / 1 080 / 1 440 that a caller without state has to make: ten
      chunks' worth of filter lines instead of four; with bound pruning on (the engine's default) and off, as the engine runs them --
      on the wide filter from its row table, one gather per k-mer instead of h -- and, for the line-count comparison, with the row
      table switched off (pruning on)
  (b) the locate pass on the whole reads: one pass over all k-mers in the plain form -- what the four feeds gather in sum
  (p) the prefix pass with the four checkpoints: the same rows where all bases are there at once

Expectation from line counts: (r) ~ (b) plus, per feed, one read and one write of the slots (64 KiB per read and feed on c3 beside
2.1 MB of gathers: about 3 %) and the k - 1 k-mers each later feed recounts across its seam; well below (c) on the wide filter.  On the
narrow filters (c) runs the clock-phased kernels and (r) the plain form.
Reported: (r)/(c), (r)/(b), (r)/(p) beside the same-setting spread of (b).

Method (measuring guide): one warm-up round, then REPS alternated rounds (r, b, p, c with pruning, c without, c without rows, r, ...), hipEvent kernel
time of rb_engine_kernel_time (summed over the four calls of (r) and of (c)), medians, min and max stated.  The rows of the four feeds
are compared with the chunked calls' before anything is timed.
usage: python profiles/resume_cost.py [--legs c3,readme] [--reps 5] [--reads 250000] [--out profiles/resume/cost.txt]

--lists: the LIST FORM of the pass (rb_resume_set_lists) instead, APPENDED to the file under a heading of its own.  Per leg, one process,
one slot set, alternated rounds of
  (r0) the four feeds under RB_PASS_LISTS_OFF
  (rl) the four feeds under the list form (RB_PASS_LISTS_BUILD: the warm-up builds the table where the filter has none; the plan's
       list_lines is printed -- 0 on the README shape, whose narrow filters do not qualify: the control, (rl)/(r0) = 1.000 expected)
  (c)  the four chunked rb_classify_batch_device_ex calls as the engine runs them today (bound pruning on, row table AUTO)
Expectation to confirm or refute on c3: a feed gathers two lines per k-mer as locate's list form does (34.4 ms per 1 M items of 360 bp),
plus 32 KiB read and 32 KiB written per item -- the first feed (FIRST) reads none.  The rows of both forms are compared before timing."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from readbouncer_amd import capi, synth  # noqa: E402

SEEDS = {"c3": (4, 40), "mock_deplete": (11, 110), "mock_t1": (12, 111), "mock_t2": (13, 112), "mock_t3": (14, 113)}
LEGS = {"c3": (["c3"], []), "readme": (["mock_deplete"], ["mock_t1", "mock_t2", "mock_t3"])}
READ_LEN = 1440
CHUNK = 360
CHECKPOINTS = (360, 720, 1080, 1440)


def kernel_ms(eng, fn):
    eng.kernel_time()  # drop what is pending
    fn()
    ms, calls = eng.kernel_time()
    assert calls >= 1
    return ms


def run_leg(name, n_reads, reps, torch, say):
    dep_keys, tgt_keys = LEGS[name]
    built = {k: synth.build_device_filter(0, synth.WORKLOADS[k], *SEEDS[k], n_segments=512 if k.startswith("mock_") else 2048) for k in dep_keys + tgt_keys}
    dep, tgt = [built[k][0] for k in dep_keys], [built[k][0] for k in tgt_keys]
    nf, P = len(dep) + len(tgt), len(CHECKPOINTS)
    eng = capi.Engine(0, dep, tgt)
    eng.set_timing(1)
    rs = eng.resume(n_reads, CHUNK, READ_LEN)
    dev = torch.device("cuda:0")
    seqs, offs, lens = synth.make_reads_device(77, n_reads, READ_LEN, built[(dep_keys + tgt_keys)[0]][1], dev)
    slots = torch.arange(n_reads, dtype=torch.int32, device=dev)
    first = torch.full((n_reads,), capi.RB_RESUME_FIRST, dtype=torch.uint8, device=dev)
    r_max, c_max = (torch.zeros((P, n_reads, nf), dtype=torch.int16, device=dev) for _ in range(2))
    r_dec, c_dec, r_st = (torch.zeros((P, n_reads), dtype=torch.uint8, device=dev) for _ in range(3))
    r_best, r_len = (torch.zeros((P, n_reads), dtype=torch.int32, device=dev) for _ in range(2))
    p_max = torch.zeros((n_reads, P, nf), dtype=torch.int16, device=dev)
    p_dec, p_st = (torch.zeros((n_reads, P), dtype=torch.uint8, device=dev) for _ in range(2))
    p_best, p_len = (torch.zeros((n_reads, P), dtype=torch.int32, device=dev) for _ in range(2))
    p_first = torch.zeros(n_reads, dtype=torch.int32, device=dev)
    loc = {k: torch.zeros((n_reads, nf), dtype=dt, device=dev) for k, dt in (("m", torch.int16), ("b", torch.int32), ("s", torch.uint8), ("h", torch.int32))}
    l_st = torch.zeros(n_reads, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def feeds():
        for p in range(P):
            rs.feed_device(seqs.data_ptr(), offs.data_ptr(), lens.data_ptr(), n_reads, slots.data_ptr(), first.data_ptr() if p == 0 else None,
                           chunk_start=p * CHUNK, chunk_length=CHUNK, d_max_count=r_max[p].data_ptr(), d_decision=r_dec[p].data_ptr(),
                           d_best_target=r_best[p].data_ptr(), d_status=r_st[p].data_ptr(), d_total_len=r_len[p].data_ptr())

    def prefixes():
        eng.prefixes_device(seqs.data_ptr(), offs.data_ptr(), lens.data_ptr(), n_reads, READ_LEN, CHECKPOINTS, d_max_count=p_max.data_ptr(),
                            d_decision=p_dec.data_ptr(), d_best_target=p_best.data_ptr(), d_status=p_st.data_ptr(), d_prefix_len=p_len.data_ptr(),
                            d_first_decided=p_first.data_ptr())

    def locate():
        eng.locate_device(seqs.data_ptr(), offs.data_ptr(), lens.data_ptr(), n_reads, READ_LEN, d_max_count=loc["m"].data_ptr(),
                          d_best_bin=loc["b"].data_ptr(), d_best_strand=loc["s"].data_ptr(), d_hit_bins=loc["h"].data_ptr(), d_status=l_st.data_ptr())

    def chunked(pruning, rows=capi.RB_ROW_TABLE_AUTO):
        def go():
            eng.set_bound_pruning(pruning)
            eng.set_row_table(rows)
            for p, c in enumerate(CHECKPOINTS):
                eng.classify_device_ex(seqs.data_ptr(), offs.data_ptr(), lens.data_ptr(), n_reads, READ_LEN, chunk_length=c,
                                       d_maxcount=c_max[p].data_ptr(), d_decision=c_dec[p].data_ptr())
            eng.set_bound_pruning(1)
            eng.set_row_table(capi.RB_ROW_TABLE_AUTO)
        return go

    legs = (("r", feeds), ("b", locate), ("p", prefixes), ("c_on", chunked(1)), ("c_off", chunked(0)), ("c_norow", chunked(1, capi.RB_ROW_TABLE_OFF)))
    for _, fn in legs:  # warm-up
        kernel_ms(eng, fn)
    torch.cuda.synchronize()
    assert torch.equal(r_max, c_max), "the feeds' maxima differ from the chunked classify calls'"
    assert torch.equal(r_dec, c_dec), "the feeds' decisions differ from the chunked classify calls'"
    assert torch.equal(r_max[P - 1], loc["m"]), "the last feed's maxima differ from the locate pass's"
    assert int(r_st.max()) == 0 and all(int(r_len[p].min()) == int(r_len[p].max()) == CHECKPOINTS[p] for p in range(P))
    ms = {key: [] for key, _ in legs}
    for _ in range(reps):  # alternated
        for key, fn in legs:
            ms[key].append(kernel_ms(eng, fn))
    med = {key: statistics.median(v) for key, v in ms.items()}
    spread_b = max(ms["b"]) - min(ms["b"])
    say("%s: %d reads of %d bp in %d chunks of %d, %d filter(s), %d slots = %.3f GB of HBM (%d bytes per slot), %d alternated repetitions" %
        (name, n_reads, READ_LEN, P, CHUNK, nf, n_reads, rs.bytes / 1e9, rs.bytes // n_reads, reps))
    for key, what in (("r", "(r) four feeds onto the slots         "), ("b", "(b) locate pass, whole reads          "),
                      ("p", "(p) prefix pass, four checkpoints     "), ("c_on", "(c) four chunked classify, pruning on "),
                      ("c_off", "(c) four chunked classify, pruning off"), ("c_norow", "(c) ... pruning on, row table off    ")):
        say("  %s: median %.3f ms  (min %.3f, max %.3f)" % (what, med[key], min(ms[key]), max(ms[key])))
    say("  (r)/(c, pruning on) = %.4f   (r)/(c, pruning off) = %.4f   (r)/(c, row table off) = %.4f   (r)/(b) = %.4f   (r)/(p) = %.4f" %
        (med["r"] / med["c_on"], med["r"] / med["c_off"], med["r"] / med["c_norow"], med["r"] / med["b"], med["r"] / med["p"]))
    say("  same-setting spread of (b) = %.3f ms (%.2f %% of its median); (r) - (b) = %.3f ms = %.1f spreads" %
        (spread_b, 100.0 * spread_b / med["b"], med["r"] - med["b"], (med["r"] - med["b"]) / spread_b if spread_b > 0 else float("inf")))
    rs.destroy()
    eng.destroy()
    for k in built:
        built[k][0].free()
    torch.cuda.empty_cache()


def run_lists_leg(name, n_reads, reps, torch, say):
    dep_keys, tgt_keys = LEGS[name]
    built = {k: synth.build_device_filter(0, synth.WORKLOADS[k], *SEEDS[k], n_segments=512 if k.startswith("mock_") else 2048) for k in dep_keys + tgt_keys}
    dep, tgt = [built[k][0] for k in dep_keys], [built[k][0] for k in tgt_keys]
    nf, P = len(dep) + len(tgt), len(CHECKPOINTS)
    eng = capi.Engine(0, dep, tgt)
    eng.set_timing(1)
    rs = eng.resume(n_reads, CHUNK, READ_LEN)
    dev = torch.device("cuda:0")
    seqs, offs, lens = synth.make_reads_device(77, n_reads, READ_LEN, built[(dep_keys + tgt_keys)[0]][1], dev)
    slots = torch.arange(n_reads, dtype=torch.int32, device=dev)
    first = torch.full((n_reads,), capi.RB_RESUME_FIRST, dtype=torch.uint8, device=dev)
    out = {key: (torch.zeros((P, n_reads, nf), dtype=torch.int16, device=dev), torch.zeros((P, n_reads), dtype=torch.uint8, device=dev))
           for key in ("r0", "rl", "c")}
    r_best, r_len = (torch.zeros((P, n_reads), dtype=torch.int32, device=dev) for _ in range(2))
    r_st = torch.zeros((P, n_reads), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def feeds(key, mode):
        def go():
            rs.set_lists(mode)
            for p in range(P):
                rs.feed_device(seqs.data_ptr(), offs.data_ptr(), lens.data_ptr(), n_reads, slots.data_ptr(), first.data_ptr() if p == 0 else None,
                               chunk_start=p * CHUNK, chunk_length=CHUNK, d_max_count=out[key][0][p].data_ptr(), d_decision=out[key][1][p].data_ptr(),
                               d_best_target=r_best[p].data_ptr(), d_status=r_st[p].data_ptr(), d_total_len=r_len[p].data_ptr())
        return go

    def chunked():
        for p, c in enumerate(CHECKPOINTS):
            eng.classify_device_ex(seqs.data_ptr(), offs.data_ptr(), lens.data_ptr(), n_reads, READ_LEN, chunk_length=c,
                                   d_maxcount=out["c"][0][p].data_ptr(), d_decision=out["c"][1][p].data_ptr())

    legs = (("r0", feeds("r0", capi.RB_PASS_LISTS_OFF)), ("rl", feeds("rl", capi.RB_PASS_LISTS_BUILD)), ("c", chunked))
    for _, fn in legs:  # warm-up (builds the list table under BUILD)
        kernel_ms(eng, fn)
    torch.cuda.synchronize()
    lines = [rs.plan(j)["list_lines"] for j in range(nf)]
    for key in ("rl", "c"):
        assert torch.equal(out["r0"][0], out[key][0]) and torch.equal(out["r0"][1], out[key][1]), "rows of (%s) differ from the plain feeds'" % key
    assert int(r_st.max()) == 0
    ms = {key: [] for key, _ in legs}
    for _ in range(reps):  # alternated
        for key, fn in legs:
            ms[key].append(kernel_ms(eng, fn))
    med = {key: statistics.median(v) for key, v in ms.items()}
    spread = {key: max(v) - min(v) for key, v in ms.items()}
    say("%s: %d reads of %d bp in %d chunks of %d, %d filter(s), %d slots = %.3f GB of HBM, list_lines per filter %s, %d alternated repetitions" %
        (name, n_reads, READ_LEN, P, CHUNK, nf, n_reads, rs.bytes / 1e9, lines, reps))
    for key, what in (("r0", "(r0) four feeds, setting off          "), ("rl", "(rl) four feeds, list form            "),
                      ("c", "(c)  four chunked classify, as today  ")):
        say("  %s: median %.3f ms  (min %.3f, max %.3f, spread %.3f)" % (what, med[key], min(ms[key]), max(ms[key]), spread[key]))
    say("  (rl)/(r0) = %.4f   (rl)/(c) = %.4f   (r0)/(c) = %.4f   (r0) - (rl) = %.3f ms = %.1f spreads of (r0)" %
        (med["rl"] / med["r0"], med["rl"] / med["c"], med["r0"] / med["c"], med["r0"] - med["rl"],
         (med["r0"] - med["rl"]) / spread["r0"] if spread["r0"] > 0 else float("inf")))
    rs.destroy()
    eng.destroy()
    for k in built:
        built[k][0].free()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="c3,readme")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reads", type=int, default=250_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resume", "cost.txt"))
    ap.add_argument("--lists", action="store_true", help="the list form against the plain feeds and the chunked calls, appended to --out")
    args = ap.parse_args()
    assert args.reps >= 5, "at least five alternated repetitions"
    import torch
    if capi.device_count() <= 0:
        sys.exit("resume_cost.py needs a GPU")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a" if args.lists else "w") as fh:
        def say(line):
            print(line, flush=True)
            fh.write(line + "\n")
            fh.flush()
        if args.lists:
            say("")
            say("resume cost, list form (rb_resume_set_lists) -- %s, library %s" % (torch.cuda.get_device_name(0), os.path.basename(capi.LIB_PATH)))
        else:
            say("resume cost -- %s, library %s" % (torch.cuda.get_device_name(0), os.path.basename(capi.LIB_PATH)))
        for leg in args.legs.split(","):
            (run_lists_leg if args.lists else run_leg)(leg.strip(), args.reads, args.reps, torch, say)


if __name__ == "__main__":
    main()
