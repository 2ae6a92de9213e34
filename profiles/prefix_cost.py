"""What the prefix pass costs: one walk over a read's k-mers with the maximum taken at every checkpoint, beside the two
things it can be held against.

  c3      config 3's filter (8 GiB, W = 128)
  readme  the README shape (four narrow filters)
both with reads of 1 440 bp and the checkpoints 360 / 720 / 1 080 / 1 440, all reads, in ONE process:
  (a) the prefix pass (rb_prefix_batch_device, every output asked for)
  (b) the locate pass on the whole reads: the same gathers in the same schedule -- the yardstick
  (c) the four rb_classify_batch_device_ex calls with chunk_length = 360 / 720 / 1 080 / 1 440 that (a) replaces: ten chunks' worth of
      filter lines instead of four; with bound pruning on (the engine's default) and off

Expectation from the code: (a) ~ (b) plus P maxima and at most one partly masked load batch per checkpoint, and well below (c).
Reported: (a)/(b) and (a)/(c) beside the same-setting spread of (b) (max - min over its repetitions); (a) - (b) in units of that spread.

Method (measuring guide): one warm-up round, then REPS alternated rounds (a, b, c with pruning, c without, a, ...), hipEvent kernel time
of rb_engine_kernel_time (summed over the four calls of (c)), medians, min and max stated.  No target: it tells a user what
--report-prefixes costs.  usage: python profiles/prefix_cost.py [--legs c3,readme] [--reps 5] [--reads 250000] [--out profiles/prefix/cost.txt]

--lists: the LIST FORM of the pass (rb_engine_set_prefix_lists) instead, APPENDED to the file under a heading of its own.  Per leg, one
process, the same reads and checkpoints, alternated rounds of
  (a)  the prefix pass under RB_PASS_LISTS_OFF
  (a') the prefix pass under the list form (RB_PASS_LISTS_BUILD: the warm-up builds the table where the filter has none; the plan's
       list_lines and the item counters are printed, and on the readme leg, where no filter qualifies, (a') launches what (a) launches)
  (b') the locate pass on the whole reads under rb_engine_set_pass_lists
  (c)  the four chunked classify calls as the engine runs them (from the list table too where the engine's policy takes it)
Reported: (a) - (a') in units of (a)'s own spread -- a gain only beyond three of them -- (a')/(b') with (a') - (b') in spreads of (b'), and
(a')/(c).  Each scan of the list form reads cnt_dwords / 256 pieces of 16 bytes per lane: 2 P of them per item."""
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
    dev = torch.device("cuda:0")
    seqs, offs, lens = synth.make_reads_device(77, n_reads, READ_LEN, built[(dep_keys + tgt_keys)[0]][1], dev)
    c_max = torch.zeros((P, n_reads, nf), dtype=torch.int16, device=dev)
    c_dec = torch.zeros((P, n_reads), dtype=torch.uint8, device=dev)
    p_max = torch.zeros((n_reads, P, nf), dtype=torch.int16, device=dev)
    p_dec, p_st = (torch.zeros((n_reads, P), dtype=torch.uint8, device=dev) for _ in range(2))
    p_best, p_len = (torch.zeros((n_reads, P), dtype=torch.int32, device=dev) for _ in range(2))
    p_first = torch.zeros(n_reads, dtype=torch.int32, device=dev)
    loc = {k: torch.zeros((n_reads, nf), dtype=dt, device=dev) for k, dt in (("m", torch.int16), ("b", torch.int32), ("s", torch.uint8), ("h", torch.int32))}
    l_st = torch.zeros(n_reads, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def prefixes():
        eng.prefixes_device(seqs.data_ptr(), offs.data_ptr(), lens.data_ptr(), n_reads, READ_LEN, CHECKPOINTS, d_max_count=p_max.data_ptr(),
                            d_decision=p_dec.data_ptr(), d_best_target=p_best.data_ptr(), d_status=p_st.data_ptr(), d_prefix_len=p_len.data_ptr(),
                            d_first_decided=p_first.data_ptr())

    def locate():
        eng.locate_device(seqs.data_ptr(), offs.data_ptr(), lens.data_ptr(), n_reads, READ_LEN, d_max_count=loc["m"].data_ptr(),
                          d_best_bin=loc["b"].data_ptr(), d_best_strand=loc["s"].data_ptr(), d_hit_bins=loc["h"].data_ptr(), d_status=l_st.data_ptr())

    def chunked(pruning):
        def go():
            eng.set_bound_pruning(pruning)
            for p, c in enumerate(CHECKPOINTS):
                eng.classify_device_ex(seqs.data_ptr(), offs.data_ptr(), lens.data_ptr(), n_reads, READ_LEN, chunk_length=c,
                                       d_maxcount=c_max[p].data_ptr(), d_decision=c_dec[p].data_ptr())
            eng.set_bound_pruning(1)
        return go

    legs = (("a", prefixes), ("b", locate), ("c_on", chunked(1)), ("c_off", chunked(0)))
    for _, fn in legs:  # warm-up
        kernel_ms(eng, fn)
    torch.cuda.synchronize()
    assert torch.equal(p_max.permute(1, 0, 2), c_max), "the prefix pass's maxima differ from the chunked classify calls'"
    assert torch.equal(p_dec.permute(1, 0), c_dec), "the prefix pass's decisions differ from the chunked classify calls'"
    assert torch.equal(p_max[:, P - 1, :], loc["m"]), "the last checkpoint's maxima differ from the locate pass's"
    ms = {key: [] for key, _ in legs}
    for _ in range(reps):  # alternated
        for key, fn in legs:
            ms[key].append(kernel_ms(eng, fn))
    med = {key: statistics.median(v) for key, v in ms.items()}
    spread_b = max(ms["b"]) - min(ms["b"])
    say("%s: %d reads of %d bp, %d filter(s), checkpoints %s, %d alternated repetitions" % (name, n_reads, READ_LEN, nf, "/".join(map(str, CHECKPOINTS)), reps))
    for key, what in (("a", "(a) prefix pass, one walk            "), ("b", "(b) locate pass, whole reads         "),
                      ("c_on", "(c) four chunked classify, pruning on "), ("c_off", "(c) four chunked classify, pruning off")):
        say("  %s: median %.3f ms  (min %.3f, max %.3f)" % (what, med[key], min(ms[key]), max(ms[key])))
    say("  (a)/(b) = %.4f   (a)/(c, pruning on) = %.4f   (a)/(c, pruning off) = %.4f" % (med["a"] / med["b"], med["a"] / med["c_on"], med["a"] / med["c_off"]))
    say("  same-setting spread of (b) = %.3f ms (%.2f %% of its median); (a) - (b) = %.3f ms = %.1f spreads" %
        (spread_b, 100.0 * spread_b / med["b"], med["a"] - med["b"], (med["a"] - med["b"]) / spread_b if spread_b > 0 else float("inf")))
    eng.destroy()
    for k in built:
        built[k][0].free()
    torch.cuda.empty_cache()


def run_leg_lists(name, n_reads, reps, torch, say):
    dep_keys, tgt_keys = LEGS[name]
    built = {k: synth.build_device_filter(0, synth.WORKLOADS[k], *SEEDS[k], n_segments=512 if k.startswith("mock_") else 2048) for k in dep_keys + tgt_keys}
    dep, tgt = [built[k][0] for k in dep_keys], [built[k][0] for k in tgt_keys]
    nf, P = len(dep) + len(tgt), len(CHECKPOINTS)
    eng = capi.Engine(0, dep, tgt)
    eng.set_timing(1)
    dev = torch.device("cuda:0")
    seqs, offs, lens = synth.make_reads_device(77, n_reads, READ_LEN, built[(dep_keys + tgt_keys)[0]][1], dev)
    c_max = torch.zeros((P, n_reads, nf), dtype=torch.int16, device=dev)
    c_dec = torch.zeros((P, n_reads), dtype=torch.uint8, device=dev)
    out = {key: (torch.zeros((n_reads, P, nf), dtype=torch.int16, device=dev), torch.zeros((n_reads, P), dtype=torch.uint8, device=dev),
                 torch.zeros((n_reads, P), dtype=torch.uint8, device=dev), torch.zeros((n_reads, P), dtype=torch.int32, device=dev),
                 torch.zeros((n_reads, P), dtype=torch.int32, device=dev), torch.zeros(n_reads, dtype=torch.int32, device=dev)) for key in ("a", "al")}
    loc = {k: torch.zeros((n_reads, nf), dtype=dt, device=dev) for k, dt in (("m", torch.int16), ("b", torch.int32), ("s", torch.uint8), ("h", torch.int32))}
    l_st = torch.zeros(n_reads, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def prefixes(key, mode):
        def go():
            eng.set_prefix_lists(mode)
            o = out[key]
            eng.prefixes_device(seqs.data_ptr(), offs.data_ptr(), lens.data_ptr(), n_reads, READ_LEN, CHECKPOINTS, d_max_count=o[0].data_ptr(),
                                d_decision=o[1].data_ptr(), d_status=o[2].data_ptr(), d_best_target=o[3].data_ptr(), d_prefix_len=o[4].data_ptr(),
                                d_first_decided=o[5].data_ptr())
        return go

    def locate():
        eng.locate_device(seqs.data_ptr(), offs.data_ptr(), lens.data_ptr(), n_reads, READ_LEN, d_max_count=loc["m"].data_ptr(),
                          d_best_bin=loc["b"].data_ptr(), d_best_strand=loc["s"].data_ptr(), d_hit_bins=loc["h"].data_ptr(), d_status=l_st.data_ptr())

    def chunked():
        for p, c in enumerate(CHECKPOINTS):
            eng.classify_device_ex(seqs.data_ptr(), offs.data_ptr(), lens.data_ptr(), n_reads, READ_LEN, chunk_length=c,
                                   d_maxcount=c_max[p].data_ptr(), d_decision=c_dec[p].data_ptr())

    eng.set_pass_lists(capi.RB_PASS_LISTS_BUILD)
    legs = (("a", prefixes("a", capi.RB_PASS_LISTS_OFF)), ("al", prefixes("al", capi.RB_PASS_LISTS_BUILD)), ("bl", locate), ("c", chunked))
    for _, fn in legs:  # warm-up (builds the list table where the filter qualifies)
        kernel_ms(eng, fn)
    eng.prefix_lists_items(reset=True)
    kernel_ms(eng, legs[1][1])
    torch.cuda.synchronize()
    listed, plain = eng.prefix_lists_items(reset=True)
    plans = [eng.plan_prefix(j, READ_LEN, CHECKPOINTS[-1])["list_lines"] for j in range(nf)]
    loc_plans = [eng.plan_pass(j, READ_LEN)["list_lines"] for j in range(nf)]
    for x, y in zip(out["a"], out["al"]):
        assert torch.equal(x, y), "the list form's outputs differ from the plain form's"
    assert torch.equal(out["al"][0].permute(1, 0, 2), c_max), "the prefix pass's maxima differ from the chunked classify calls'"
    assert torch.equal(out["al"][0][:, P - 1, :], loc["m"]), "the last checkpoint's maxima differ from the locate pass's"
    ms = {key: [] for key, _ in legs}
    for _ in range(reps):  # alternated
        for key, fn in legs:
            ms[key].append(kernel_ms(eng, fn))
    med = {key: statistics.median(v) for key, v in ms.items()}
    spread = {key: max(v) - min(v) for key, v in ms.items()}
    say("%s: %d reads of %d bp, %d filter(s), checkpoints %s, %d alternated repetitions" % (name, n_reads, READ_LEN, nf, "/".join(map(str, CHECKPOINTS)), reps))
    say("  plan_prefix list_lines per filter %s (plan_pass %s); one call under the list form: %d items listed, %d plain" % (plans, loc_plans, listed, plain))
    for key, what in (("a", "(a)  prefix pass, RB_PASS_LISTS_OFF     "), ("al", "(a') prefix pass, list form             "),
                      ("bl", "(b') locate pass, list form, whole reads"), ("c", "(c)  four chunked classify, as planned  ")):
        say("  %s: median %.3f ms  (min %.3f, max %.3f)" % (what, med[key], min(ms[key]), max(ms[key])))
    say("  (a')/(a) = %.4f   (a')/(b') = %.4f   (a')/(c) = %.4f" % (med["al"] / med["a"], med["al"] / med["bl"], med["al"] / med["c"]))
    say("  spread of (a) = %.3f ms; (a) - (a') = %.3f ms = %.1f spreads of (a)" %
        (spread["a"], med["a"] - med["al"], (med["a"] - med["al"]) / spread["a"] if spread["a"] > 0 else float("inf")))
    say("  spread of (b') = %.3f ms; (a') - (b') = %.3f ms = %.1f spreads of (b')" %
        (spread["bl"], med["al"] - med["bl"], (med["al"] - med["bl"]) / spread["bl"] if spread["bl"] > 0 else float("inf")))
    eng.destroy()
    for k in built:
        built[k][0].free()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="c3,readme")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reads", type=int, default=250_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prefix", "cost.txt"))
    ap.add_argument("--lists", action="store_true", help="the list form's block, appended to --out")
    args = ap.parse_args()
    assert args.reps >= 5, "at least five alternated repetitions"
    import torch
    if capi.device_count() <= 0:
        sys.exit("prefix_cost.py needs a GPU")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a" if args.lists else "w") as fh:
        def say(line):
            print(line, flush=True)
            fh.write(line + "\n")
            fh.flush()
        if args.lists:
            say("")
            say("prefix cost, list form (rb_engine_set_prefix_lists) -- %s, library %s" % (torch.cuda.get_device_name(0), os.path.basename(capi.LIB_PATH)))
        else:
            say("prefix cost -- %s, library %s" % (torch.cuda.get_device_name(0), os.path.basename(capi.LIB_PATH)))
        for leg in args.legs.split(","):
            (run_leg_lists if args.lists else run_leg)(leg.strip(), args.reads, args.reps, torch, say)


if __name__ == "__main__":
    main()
