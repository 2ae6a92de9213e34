#!/usr/bin/env python3
"""The wide list form of the plain count kernel (rb_engine_set_wide_lists: ibf_count_wide_lists_kernel on the filter's wide list table)
against the plain kernel (the setting OFF), alternated in one process, on the filter of bench leg grch38_f100k (synth.WORKLOADS: GRCh38
at fragment_size 100 000, about 31 000 bins, W = 485, 4.8 GB, built once with bench.py's seeds) for three read mixes of 360 bp: the
bench's (50 % positives), all positive and all negative.  Reports the count kernels' ms per 1 M reads (hipEvent pairs,
rb_engine_set_timing), median of the repeats, checks that raw maxima, decisions and status are identical in both modes, and what the
table cost: bytes, lines per slot, the census, overflow rows, allocation seconds, build milliseconds (census included), and the first
call with the build in it against the second without.

  python3 profiles/wide_lists_cost.py [reads per launch, default 1000000] [repeats, default 5] [--out FILE]
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
n_reads = int(args[0]) if len(args) > 0 else 1_000_000
reps = int(args[1]) if len(args) > 1 else 5
L = 360
MODES = (("off", capi.RB_PASS_LISTS_OFF), ("build", capi.RB_PASS_LISTS_BUILD))
lines_out = []


def say(*parts):
    line = " ".join(str(p) for p in parts)
    print(line, flush=True)
    lines_out.append(line)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write("\n".join(lines_out) + "\n")


def heartbeat():  # (the build of a 48 GiB table says nothing for minutes; a line a minute shows that the run is alive)
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
say("filter", json.dumps({k: int(v) for k, v in d.info.items()}))


def launch(mode, batch, timed=True):
    t_seq, t_off, t_len = batch
    eng.set_wide_lists(mode)
    t_max = torch.zeros((n_reads, 1), dtype=torch.int16, device=dev)
    t_dec = torch.zeros(n_reads, dtype=torch.uint8, device=dev)
    t_st = torch.zeros(n_reads, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    eng.set_timing(timed)
    t0 = time.perf_counter()
    eng.classify_device(t_seq.data_ptr(), t_off.data_ptr(), t_len.data_ptr(), n_reads, L, 0.1, 0.95, capi.RB_MODE_CHECK_UNBLOCK,
                        t_max.data_ptr(), None, t_dec.data_ptr(), t_st.data_ptr())
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    k_ms = eng.kernel_time()[0] if timed else 0.0
    eng.set_timing(False)
    return k_ms, wall, (t_max.cpu(), t_dec.cpu(), t_st.cpu())


bench_mix = synth.make_reads_device(1000, n_reads, L, ref, dev, positive_fraction=0.5)
say("plan off", eng.plan(0, n_reads, L)["kernel"])
launch(capi.RB_PASS_LISTS_OFF, bench_mix, timed=False)  # warm-up
_, first_wall, _ = launch(capi.RB_PASS_LISTS_BUILD, bench_mix, timed=False)  # builds the wide list table
_, second_wall, _ = launch(capi.RB_PASS_LISTS_BUILD, bench_mix, timed=False)
info = d.wide_list_table_info()
cost = {"bytes": info["bytes"], "rows": info["rows"], "lines": info["lines"], "side_rows": info["side_rows"], "side_bytes": info["side_bytes"],
        "census_rows": info["census_rows"], "census_over_256_384_512": info["census_over"], "refused": info["refused"],
        "alloc_s": round(info["alloc_s"], 4), "build_ms": round(info["build_ms"], 2), "first_build_call_s": round(first_wall, 4),
        "second_build_call_s": round(second_wall, 4), "plan": eng.plan(0, n_reads, L)["kernel"]}
say("table", json.dumps(cost))

res = {}
for mix, pos in (("bench", 0.5), ("positive", 1.0), ("negative", 0.0)):
    batch = bench_mix if mix == "bench" else synth.make_reads_device(1000, n_reads, L, ref, dev, positive_fraction=pos)
    outs, ms = {}, {m: [] for m, _ in MODES}
    for rep in range(reps + 1):  # the first round warms up and is not counted
        for name, mode in (MODES[::-1] if rep % 2 else MODES):
            k_ms, _, o = launch(mode, batch)
            if rep:
                ms[name].append(k_ms * 1e6 / n_reads)
            if name in outs:
                assert all(torch.equal(a, b) for a, b in zip(outs[name], o)), (mix, name, "repeat differs")
            outs[name] = o
    same = all(torch.equal(a, b) for a, b in zip(outs["off"], outs["build"]))
    med = {m: statistics.median(v) for m, v in ms.items()}
    res[mix] = {"ms_per_1M": {m: round(v, 3) for m, v in med.items()}, "spread": {m: round((max(v) - min(v)) / med[m], 4) for m, v in ms.items()},
                "off_over_build": round(med["off"] / med["build"], 4), "outputs_identical": same,
                "runs": {m: [round(x, 3) for x in v] for m, v in ms.items()}}
    say(mix, json.dumps(res[mix]))
    assert same, mix
say(json.dumps({"workload": "grch38_f100k", "reads_per_launch": n_reads, "read_len": L, "table": cost, "mixes": res}))
