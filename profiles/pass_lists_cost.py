"""What locate and hits cost from the list table (rb_engine_set_pass_lists) beside the plain form on the same reads,
the same filter and the same engine, in one process.

  c3      config 3's filter as bench.py synthesises it (8 GiB, W = 128), list table built first; 1 M work items of 360 bp.  Alternated:
          locate plain, locate lists, hits plain, hits lists (min_count = 0, max_hits = 64), and the list COUNT kernel with bound pruning
          off -- the same gathers and adds with the plain maximum scan, so list locate / unpruned list count is what the richer scans cost.
  readme  the README shape (four narrow filters): none qualifies, so the two settings run the same kernels and the ratio is the run's
          noise -- the control.

Method (measuring guide): one warm-up round, then REPS alternated rounds, hipEvent time of rb_engine_kernel_time, medians with the spread
(min-max) stated.  The criterion is relative to the plain form of the same run.  usage: python profiles/pass_lists_cost.py
[--legs c3,readme] [--reps 7] [--reads 1000000] [--out profiles/pass_lists/cost.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from readbouncer_amd import capi, synth  # noqa: E402
from profiles.hits_cost import LEGS, SEEDS, kernel_ms  # noqa: E402

MAX_HITS = 64


def run_leg(name, n_reads, reps, torch, say):
    dep_keys, tgt_keys, read_len = LEGS[name]
    built = {k: synth.build_device_filter(0, synth.WORKLOADS[k], *SEEDS[k], n_segments=512 if k.startswith("mock_") else 2048) for k in dep_keys + tgt_keys}
    dep, tgt = [built[k][0] for k in dep_keys], [built[k][0] for k in tgt_keys]
    nf = len(dep) + len(tgt)
    infos = [d.list_table_build() for d in dep + tgt]
    eng = capi.Engine(0, dep, tgt)
    eng.set_timing(1)
    dev = torch.device("cuda:0")
    seqs, offs, lens = synth.make_reads_device(77, n_reads, read_len, built[(dep_keys + tgt_keys)[0]][1], dev)
    n_bins = sum(int(d.info["n_bins"]) for d in dep + tgt)
    out = {k: torch.zeros((n_reads, nf), dtype=dt, device=dev) for k, dt in (("m", torch.int16), ("b", torch.int32), ("s", torch.uint8), ("h", torch.int32))}
    t_hits = torch.zeros((n_reads, nf, MAX_HITS, 2), dtype=torch.int32, device=dev)
    t_n = torch.zeros((n_reads, nf), dtype=torch.int32, device=dev)
    t_bins = torch.zeros(n_bins, dtype=torch.int64, device=dev)
    t_st = torch.zeros(n_reads, dtype=torch.uint8, device=dev)
    t_mc = torch.zeros((n_reads, nf), dtype=torch.int16, device=dev)
    torch.cuda.synchronize()

    def locate():
        eng.locate_device(seqs.data_ptr(), offs.data_ptr(), lens.data_ptr(), n_reads, read_len, d_max_count=out["m"].data_ptr(),
                          d_best_bin=out["b"].data_ptr(), d_best_strand=out["s"].data_ptr(), d_hit_bins=out["h"].data_ptr(), d_status=t_st.data_ptr())

    def hits():
        eng.hits_device(seqs.data_ptr(), offs.data_ptr(), lens.data_ptr(), n_reads, read_len, min_count=0, max_hits=MAX_HITS,
                        d_hits=t_hits.data_ptr(), d_n_hits=t_n.data_ptr(), d_status=t_st.data_ptr(), d_bin_reads=t_bins.data_ptr())

    def count():
        eng.classify_device(seqs.data_ptr(), offs.data_ptr(), lens.data_ptr(), n_reads, read_len, d_maxcount=t_mc.data_ptr())

    def with_setting(mode, fn):
        eng.set_pass_lists(mode)
        return kernel_ms(eng, fn)

    lists = [eng.plan_pass(j, read_len)["list_lines"] for j in range(nf)]
    eng.set_pass_lists(capi.RB_PASS_LISTS_CURRENT)
    lists_on = [eng.plan_pass(j, read_len)["list_lines"] for j in range(nf)]
    serves = any(lists_on)
    if serves:  # the unpruned list count kernel of the same run
        eng.set_row_table(capi.RB_ROW_TABLE_LISTS)
        eng.set_bound_pruning(0)
        assert eng.plan(0, n_reads, read_len)["kernel"] == "ibf_count_lists_kernel"
    legs = [("locate plain", capi.RB_PASS_LISTS_OFF, locate), ("locate lists", capi.RB_PASS_LISTS_CURRENT, locate),
            ("hits plain", capi.RB_PASS_LISTS_OFF, hits), ("hits lists", capi.RB_PASS_LISTS_CURRENT, hits)]
    if serves:
        legs.append(("count lists, no bound", capi.RB_PASS_LISTS_OFF, count))
    for _, mode, fn in legs:  # warm-up
        with_setting(mode, fn)
    # the outputs of the two forms, once: the same bytes
    with_setting(capi.RB_PASS_LISTS_OFF, locate)
    plain = {k: v.clone() for k, v in out.items()}
    with_setting(capi.RB_PASS_LISTS_CURRENT, locate)
    same = all(bool(torch.equal(plain[k], out[k])) for k in out)
    ms = {label: [] for label, _, _ in legs}
    for _ in range(reps):  # alternated
        for label, mode, fn in legs:
            ms[label].append(with_setting(mode, fn))
    torch.cuda.synchronize()
    pairs = n_reads * nf
    say("%s: %d work items of %d bp, %d filter(s), list_lines per filter off %s / current %s (list table lines %s), hits at min_count 0, max_hits %d, "
        "%d alternated repetitions; locate outputs of the two forms equal: %s" %
        (name, n_reads, read_len, nf, lists, lists_on, [i["lines"] for i in infos], MAX_HITS, reps, same))
    med = {}
    for label, _, _ in legs:
        per_m = [x * 1e6 / pairs for x in ms[label]]
        med[label] = statistics.median(per_m)
        say("  %-22s per 1 M (item, filter) pairs: median %.3f ms  (min %.3f, max %.3f)" % (label, med[label], min(per_m), max(per_m)))
    say("  locate lists / plain = %.4f" % (med["locate lists"] / med["locate plain"]))
    say("  hits lists / plain   = %.4f" % (med["hits lists"] / med["hits plain"]))
    if serves:
        say("  locate lists / count lists without the bound = %.4f   (what the richer scans cost)" % (med["locate lists"] / med["count lists, no bound"]))
    else:
        say("  (no filter of this leg qualifies for the list form: the control, both settings run the plain kernels)")
    eng.destroy()
    for k in built:
        built[k][0].free()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="c3,readme")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pass_lists", "cost.txt"))
    args = ap.parse_args()
    assert args.reps >= 5, "at least five alternated repetitions"
    import torch
    if capi.device_count() <= 0:
        sys.exit("pass_lists_cost.py needs a GPU")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        def say(line):
            print(line, flush=True)
            fh.write(line + "\n")
            fh.flush()
        say("pass lists cost -- %s, library %s" % (torch.cuda.get_device_name(0), os.path.basename(capi.LIB_PATH)))
        for leg in args.legs.split(","):
            run_leg(leg.strip(), args.reads, args.reps, torch, say)


if __name__ == "__main__":
    main()
