#!/usr/bin/env python3
"""The wide list forms of locate and hits (rb_engine_set_wide_pass_lists: ibf_locate_wide_lists_kernel / ibf_hits_wide_lists_kernel on
the filter's wide list table) against the plain forms (the setting OFF), alternated in one process, on the filter of bench leg
grch38_f100k (synth.WORKLOADS: GRCh38 at fragment_size 100 000, about 31 000 bins, W = 485, built once with bench.py's seeds) for three
mixes of 360 bp items: the bench's (50 % positives), all positive and all negative.  Locate, and hits at min_count 0 (the decision
threshold) with max_hits 64; in the same rounds the wide classify K1 (rb_engine_set_wide_lists, the count kernel alone), so that the
scans' cost on top of the count is visible.  Reports the calls' kernel time in ms per 1 M items (hipEvent pairs, rb_engine_set_timing:
for a pass that is every kernel of the call -- prep, the plain launch over the items left, the wide kernel, the merge), median of the
repeats with the spread, and checks that every output is byte-identical with the setting off and on.

  python3 profiles/wide_pass_lists_cost.py [items per launch, default 1000000] [repeats, default 5] [--out FILE]
"""
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from readbouncer_amd import capi, synth  # noqa: E402

argv = sys.argv[1:]
out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
args = [a for i, a in enumerate(argv) if a != "--out" and (i == 0 or argv[i - 1] != "--out")]
n = int(args[0]) if len(args) > 0 else 1_000_000
reps = int(args[1]) if len(args) > 1 else 5
L, CAP = 360, 64
OFF, CURRENT, BUILD = capi.RB_PASS_LISTS_OFF, capi.RB_PASS_LISTS_CURRENT, capi.RB_PASS_LISTS_BUILD
lines_out = []


def say(*parts):
    line = " ".join(str(p) for p in parts)
    print(line, flush=True)
    lines_out.append(line)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write("\n".join(lines_out) + "\n")


def heartbeat():  # (the build of a 48 GiB table says nothing for a while; a line a minute shows that the run is alive)
    t0 = time.time()
    while True:
        time.sleep(60)
        print("... %d s" % (time.time() - t0), file=sys.stderr, flush=True)


threading.Thread(target=heartbeat, daemon=True).start()
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
eng.set_wide_lists(CURRENT)  # the classify leg: the wide count kernel
say("plan classify", eng.plan(0, n, L)["kernel"], "; plain pass slices", eng.plan_pass(0, L)["column_slices"])

out = {"m": torch.zeros((n, 1), dtype=torch.int16, device=dev), "b": torch.zeros((n, 1), dtype=torch.int32, device=dev),
       "s": torch.zeros((n, 1), dtype=torch.uint8, device=dev), "h": torch.zeros((n, 1), dtype=torch.int32, device=dev),
       "st": torch.zeros(n, dtype=torch.uint8, device=dev), "hits": torch.zeros((n, 1, CAP, 8), dtype=torch.uint8, device=dev),
       "nh": torch.zeros((n, 1), dtype=torch.int32, device=dev), "hst": torch.zeros(n, dtype=torch.uint8, device=dev),
       "max": torch.zeros((n, 1), dtype=torch.int16, device=dev), "dec": torch.zeros(n, dtype=torch.uint8, device=dev)}


def timed(fn, keys):
    for k in keys:
        out[k].fill_(0x5A if out[k].dtype == torch.uint8 else 0)
    torch.cuda.synchronize()
    eng.kernel_time()  # drop what is pending
    fn()
    torch.cuda.synchronize()
    ms, calls = eng.kernel_time()
    assert calls >= 1
    return ms, tuple(out[k].cpu() for k in keys)


def legs(batch):
    seq, off, ln = batch

    def locate():
        eng.locate_device(seq.data_ptr(), off.data_ptr(), ln.data_ptr(), n, L, d_max_count=out["m"].data_ptr(), d_best_bin=out["b"].data_ptr(),
                          d_best_strand=out["s"].data_ptr(), d_hit_bins=out["h"].data_ptr(), d_status=out["st"].data_ptr())

    def hits():
        eng.hits_device(seq.data_ptr(), off.data_ptr(), ln.data_ptr(), n, L, min_count=0, max_hits=CAP, d_hits=out["hits"].data_ptr(),
                        d_n_hits=out["nh"].data_ptr(), d_status=out["hst"].data_ptr())

    def classify():
        eng.classify_device(seq.data_ptr(), off.data_ptr(), ln.data_ptr(), n, L, 0.1, 0.95, capi.RB_MODE_CHECK_UNBLOCK, out["max"].data_ptr(), None,
                            out["dec"].data_ptr(), None)

    return {"locate": (locate, ("m", "b", "s", "h", "st")), "hits": (hits, ("hits", "nh", "hst")), "classify_wide_k1": (classify, ("max", "dec"))}


res = {}
for mix, pos in (("bench", 0.5), ("positive", 1.0), ("negative", 0.0)):
    batch = synth.make_reads_device(1000, n, L, ref, dev, positive_fraction=pos)
    L_ = legs(batch)
    ms = {(leg, mode): [] for leg in ("locate", "hits") for mode in ("off", "current")}
    k1, outs = [], {}
    for rep in range(reps + 1):  # the first round warms up and is not counted
        order = (("off", OFF), ("current", CURRENT))
        for name, mode in (order[::-1] if rep % 2 else order):
            eng.set_wide_pass_lists(mode)
            assert eng.wide_pass_lines(0, L) == (info["lines"] if mode == CURRENT else 0)
            for leg in ("locate", "hits"):
                t, o = timed(*L_[leg])
                if rep:
                    ms[(leg, name)].append(t * 1e6 / n)
                if (leg, name) in outs:
                    assert all(torch.equal(a, b) for a, b in zip(outs[(leg, name)], o)), (mix, leg, name, "repeat differs")
                outs[(leg, name)] = o
        t, o = timed(*L_["classify_wide_k1"])
        if rep:
            k1.append(t * 1e6 / n)
    same = all(torch.equal(a, b) for leg in ("locate", "hits") for a, b in zip(outs[(leg, "off")], outs[(leg, "current")]))
    k1_med = statistics.median(k1)
    row = {"outputs_identical": same, "wide_classify_k1_ms_per_1M": round(k1_med, 3), "k1_spread": round((max(k1) - min(k1)) / k1_med, 4),
           "located": int((outs[("locate", "off")][0] != 0).sum()), "hits_total": int(outs[("hits", "off")][1].sum())}
    for leg in ("locate", "hits"):
        med = {m: statistics.median(ms[(leg, m)]) for m in ("off", "current")}
        row[leg] = {"ms_per_1M": {m: round(v, 3) for m, v in med.items()},
                    "spread": {m: round((max(ms[(leg, m)]) - min(ms[(leg, m)])) / med[m], 4) for m in med},
                    "off_over_current": round(med["off"] / med["current"], 3), "current_over_wide_k1": round(med["current"] / k1_med, 4),
                    "runs": {m: [round(x, 3) for x in ms[(leg, m)]] for m in med}}
    res[mix] = row
    say(mix, json.dumps(row))
    assert same, mix
say(json.dumps({"workload": "grch38_f100k", "items_per_launch": n, "item_len": L, "min_count": 0, "max_hits": CAP, "repeats": reps, "mixes": res}))
