#!/usr/bin/env python3
"""The lead line of bound pruning (bit 3 of rb_engine_set_prune_parts) against the state before it, alternated in one process, on config
3's filter (8 GiB, 8192 bins, built once with bench.py's seeds) for three read mixes of 360 bp: the bench's (50 % positives), all positive
(host depletion) and all negative.  Settings: mask 7 (sub-tile checks, strand lead, certificate), mask 15 (+ the lead line with the
engine's own lead_min) and mask 15 with lead_min given (rb_engine_set_lead_min: "15/6" is a lead_min of 6).  Reports the count kernel's ms
per 1 M reads (hipEvent pairs, rb_engine_set_timing), median of the repeats, checks that raw maxima, decisions and status are identical
under every setting, and reads the kernel's trace (rb_engine_set_prune_trace) for what the waves did: share of reads that took the line,
whose other lanes were certified, whose certificate held, and the same for the trailing strand.

  python3 profiles/lead_line_ab.py [reads per launch, default 1000000] [repeats, default 5] [workload of synth.WORKLOADS, default c3]
  python3 profiles/lead_line_ab.py --pmc [reads per launch]    one launch per setting on the bench mix, in the order printed (for a
                                                               counter pass of rocprofv3 around it: dispatches map to settings)
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from readbouncer_amd import capi, synth  # noqa: E402

args = [a for a in sys.argv[1:] if a != "--pmc"]
pmc = "--pmc" in sys.argv[1:]
n_reads = int(args[0]) if len(args) > 0 else 1_000_000
reps = 1 if pmc else (int(args[1]) if len(args) > 1 else 5)
workload = args[2] if len(args) > 2 else "c3"
L, K = 360, 13
SETTINGS = ("7", "15", "15/6", "15/12")
dev = torch.device("cuda:0")
d, ref = synth.build_device_filter(0, synth.WORKLOADS[workload], fill_seed=4, plant_seed=40)
torch.cuda.synchronize()
eng = capi.Engine(0, [d], [])
eng.set_split_threshold(0)
slices = eng.plan(0, n_reads, L)["column_slices"]
t_trace = torch.zeros(n_reads * slices, dtype=torch.int64, device=dev)
torch.cuda.synchronize()


def launch(setting, batch, timed=True):
    t_seq, t_off, t_len = batch
    mask, _, lead_min = setting.partition("/")
    eng.set_prune_parts(int(mask))
    eng.set_lead_min(0, int(lead_min) if lead_min else -1)
    t_max = torch.zeros((n_reads, 1), dtype=torch.int16, device=dev)
    t_best = torch.zeros(n_reads, dtype=torch.int32, device=dev)
    t_dec = torch.zeros(n_reads, dtype=torch.uint8, device=dev)
    t_st = torch.zeros(n_reads, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    eng.set_timing(timed)
    eng.classify_device(t_seq.data_ptr(), t_off.data_ptr(), t_len.data_ptr(), n_reads, L, 0.1, 0.95, capi.RB_MODE_CHECK_UNBLOCK,
                        t_max.data_ptr(), t_best.data_ptr(), t_dec.data_ptr(), t_st.data_ptr())
    k_ms = eng.kernel_time()[0] if timed else 0.0
    eng.set_timing(False)
    torch.cuda.synchronize()
    return k_ms, (t_max.cpu(), t_dec.cpu(), t_st.cpu())


def trace_summary(setting, batch):
    """one untimed launch with the trace on"""
    t_trace.zero_()
    torch.cuda.synchronize()
    eng.set_prune_trace(t_trace.data_ptr())
    launch(setting, batch, timed=False)
    eng.set_prune_trace(None)
    r = t_trace.cpu()
    f = lambda sh, m: ((r >> sh) & m).double()
    return {"led_by_reverse": round(f(0, 1).mean().item(), 4), "probed": round(f(1, 1).mean().item(), 4),
            "cert_tried": round(f(2, 1).mean().item(), 4), "cert_held": round(f(3, 1).mean().item(), 4),
            "line_taken": round(f(4, 1).mean().item(), 4), "line_cert_tried": round(f(5, 1).mean().item(), 4),
            "line_cert_held": round(f(6, 1).mean().item(), 4),
            "kmers_in_full_fwd": round(f(16, 0xFFFF).mean().item(), 1), "kmers_in_full_rev": round(f(32, 0xFFFF).mean().item(), 1)}


if pmc:
    batch = synth.make_reads_device(1000, n_reads, L, ref, dev, positive_fraction=0.5)
    launch("7", batch, timed=False)  # warm-up (measures the filter's load)
    order = []
    for s in SETTINGS + SETTINGS:
        launch(s, batch, timed=False)
        order.append(s)
    print(json.dumps({"count_kernel_dispatches_after_warm_up": order, "reads_per_launch": n_reads}))
    sys.exit(0)

res = {}
for mix, pos in (("bench", 0.5), ("positive", 1.0), ("negative", 0.0)):
    batch = synth.make_reads_device(1000, n_reads, L, ref, dev, positive_fraction=pos)
    outs, ms = {}, {s: [] for s in SETTINGS}
    for rep in range(reps + 1):  # the first round warms up and is not counted
        for s in (SETTINGS[::-1] if rep % 2 else SETTINGS):
            k_ms, o = launch(s, batch)
            if rep:
                ms[s].append(k_ms * 1e6 / n_reads)
            if s in outs:
                assert all(torch.equal(a, b) for a, b in zip(outs[s], o)), (mix, s, "repeat differs")
            outs[s] = o
    same = all(all(torch.equal(a, b) for a, b in zip(outs["7"], outs[s])) for s in SETTINGS)
    med = {s: statistics.median(ms[s]) for s in SETTINGS}
    res[mix] = {"ms_per_1M": {str(s): round(med[s], 3) for s in SETTINGS},
                "spread": {str(s): round((max(ms[s]) - min(ms[s])) / med[s], 4) for s in SETTINGS},
                "against_mask_7": {str(s): round(med["7"] / med[s], 4) for s in SETTINGS},
                "outputs_identical": same, "runs": {str(s): [round(x, 3) for x in ms[s]] for s in SETTINGS},
                "trace": {str(s): trace_summary(s, batch) for s in SETTINGS}}
    print(mix, json.dumps(res[mix]), flush=True)
    assert same, mix
    del batch
print(json.dumps({"workload": workload, "column_slices": slices, "reads_per_launch": n_reads, "read_len": L, "mixes": res}))
