#!/usr/bin/env python3
"""Bound pruning of the plain count kernel (rb_engine_set_bound_pruning) on and off, alternated, on config 3's filter (8 GiB, 8192 bins,
built once with bench.py's seeds) for three read mixes of 360 bp: the bench's (50 % positives), all positive (host depletion) and all
negative.  Reports the count kernel's ms per 1 M reads (hipEvent pairs, rb_engine_set_timing) per mix and setting, and checks that the
raw maxima, decisions and status are identical with and without pruning.

  python3 profiles/bound_pruning_ab.py [reads per launch, default 1000000] [repeats, default 5]
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from readbouncer_amd import capi, synth  # noqa: E402

n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
L = 360
dev = torch.device("cuda:0")
d, ref = synth.build_device_filter(0, synth.WORKLOADS["c3"], fill_seed=4, plant_seed=40)
torch.cuda.synchronize()
eng = capi.Engine(0, [d], [])
res = {}
for mix, pos in (("bench", 0.5), ("positive", 1.0), ("negative", 0.0)):
    t_seq, t_off, t_len = synth.make_reads_device(1000, n_reads, L, ref, dev, positive_fraction=pos)
    outs, ms = {}, {0: [], 1: []}
    for rep in range(reps + 1):  # the first round warms up and is not counted
        for on in (1, 0) if rep % 2 else (0, 1):
            eng.set_bound_pruning(on)
            t_max = torch.zeros((n_reads, 1), dtype=torch.int16, device=dev)
            t_best = torch.zeros(n_reads, dtype=torch.int32, device=dev)
            t_dec = torch.zeros(n_reads, dtype=torch.uint8, device=dev)
            t_st = torch.zeros(n_reads, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            eng.set_timing(True)
            eng.classify_device(t_seq.data_ptr(), t_off.data_ptr(), t_len.data_ptr(), n_reads, L, 0.1, 0.95, capi.RB_MODE_CHECK_UNBLOCK,
                                t_max.data_ptr(), t_best.data_ptr(), t_dec.data_ptr(), t_st.data_ptr())
            k_ms, _ = eng.kernel_time()
            eng.set_timing(False)
            torch.cuda.synchronize()
            if rep:
                ms[on].append(k_ms * 1e6 / n_reads)
            o = (t_max.cpu(), t_dec.cpu(), t_st.cpu())
            if on in outs:
                assert all(torch.equal(a, b) for a, b in zip(outs[on], o)), (mix, on, "repeat differs")
            outs[on] = o
    same = all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))
    off, on = statistics.median(ms[0]), statistics.median(ms[1])
    res[mix] = {"ms_per_1M_off": round(off, 3), "ms_per_1M_on": round(on, 3), "speedup": round(off / on, 4),
                "spread_off": round((max(ms[0]) - min(ms[0])) / off, 4), "spread_on": round((max(ms[1]) - min(ms[1])) / on, 4),
                "outputs_identical": same, "runs_off": [round(x, 3) for x in ms[0]], "runs_on": [round(x, 3) for x in ms[1]]}
    print(mix, json.dumps(res[mix]), flush=True)
    assert same, mix
    del t_seq, t_off, t_len
print(json.dumps({"reads_per_launch": n_reads, "read_len": L, "mixes": res}))
