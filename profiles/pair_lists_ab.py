#!/usr/bin/env python3
"""The pair form of the plain count kernel (RB_ROW_TABLE_PAIRS: ibf_count_pair_lists_kernel on the filter's pair table) against the list
form (RB_ROW_TABLE_LISTS: ibf_count_lists_kernel on its list table), alternated in one process, on config 3's filter (8 GiB, 8192 bins,
built once with bench.py's seeds) for three read mixes of 360 bp: the bench's (50 % positives), all positive and all negative.  Reports
the count kernels' ms per 1 M reads (hipEvent pairs, rb_engine_set_timing; either form's two launches together), median of the repeats,
checks that raw maxima, decisions and status are identical in both modes, and what the pair table cost: bytes, tail lines and dense rows
in use, allocation seconds, build milliseconds (census included), the first call with the build in it against the second without, and
the device memory in use with the filter alone, with the list table and with both tables.

  python3 profiles/pair_lists_ab.py [reads per launch, default 1000000] [repeats, default 5]
  python3 profiles/pair_lists_ab.py --pmc [reads per launch]   one launch per mode on the bench mix, in the order printed (for a counter
                                                               pass of rocprofv3 around it: dispatches map to modes)
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from readbouncer_amd import capi, synth  # noqa: E402

args = [a for a in sys.argv[1:] if a != "--pmc"]
pmc = "--pmc" in sys.argv[1:]
n_reads = int(args[0]) if len(args) > 0 else 1_000_000
reps = 1 if pmc else (int(args[1]) if len(args) > 1 else 5)
L = 360
MODES = (("lists", capi.RB_ROW_TABLE_LISTS), ("pairs", capi.RB_ROW_TABLE_PAIRS))
dev = torch.device("cuda:0")
d, ref = synth.build_device_filter(0, synth.WORKLOADS["c3"], fill_seed=4, plant_seed=40)
torch.cuda.synchronize()


def in_use():
    free, total = torch.cuda.mem_get_info(0)
    return total - free


hbm = {"filter": in_use()}
eng = capi.Engine(0, [d], [])
eng.set_split_threshold(0)


def launch(mode, batch, timed=True):
    t_seq, t_off, t_len = batch
    eng.set_row_table(mode)
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
launch(capi.RB_ROW_TABLE_LISTS, bench_mix, timed=False)  # warm-up (builds the list table)
hbm["with_list_table"] = in_use()
_, first_wall, _ = launch(capi.RB_ROW_TABLE_PAIRS, bench_mix, timed=False)  # builds the pair table
_, second_wall, _ = launch(capi.RB_ROW_TABLE_PAIRS, bench_mix, timed=False)
hbm["with_both_tables"] = in_use()
info, linfo = d.pair_table_info(), d.list_table_info()
cost = {"bytes": info["bytes"], "rows": info["rows"], "lines": info["lines"], "tail_rows": info["tail_rows"], "tail_bytes": info["tail_bytes"],
        "side_rows": info["side_rows"], "side_bytes": info["side_bytes"], "census_over": info["census_over"], "census_one_line": info["census_one_line"],
        "refused": info["refused"], "alloc_s": round(info["alloc_s"], 4), "build_ms": round(info["build_ms"], 2),
        "list_table": {"bytes": linfo["bytes"], "lines": linfo["lines"], "alloc_s": round(linfo["alloc_s"], 4), "build_ms": round(linfo["build_ms"], 2)},
        "first_pairs_call_s": round(first_wall, 4), "second_pairs_call_s": round(second_wall, 4), "plan": eng.plan(0, n_reads, L)["kernel"],
        "device_bytes_in_use": hbm}
print("table", json.dumps(cost), flush=True)

if pmc:
    order = []
    for name, mode in MODES + MODES:
        launch(mode, bench_mix, timed=False)
        order.append(name)
    print(json.dumps({"count_kernel_dispatches_after_warm_up": order, "either_form_is_two_dispatches": True, "reads_per_launch": n_reads}))
    sys.exit(0)

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
    same = all(torch.equal(a, b) for a, b in zip(outs["lists"], outs["pairs"]))
    med = {m: statistics.median(v) for m, v in ms.items()}
    res[mix] = {"ms_per_1M": {m: round(v, 3) for m, v in med.items()}, "spread": {m: round((max(v) - min(v)) / med[m], 4) for m, v in ms.items()},
                "pairs_over_lists": round(med["pairs"] / med["lists"], 4), "outputs_identical": same,
                "runs": {m: [round(x, 3) for x in v] for m, v in ms.items()}}
    print(mix, json.dumps(res[mix]), flush=True)
    assert same, mix
print(json.dumps({"workload": "c3", "reads_per_launch": n_reads, "read_len": L, "table": cost, "mixes": res}))
