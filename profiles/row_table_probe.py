#!/usr/bin/env python3
"""Step 0 of the per-k-mer row table: does the no-compute gather probe (rb_dibf_probe_read_peak, rb_probe.hip) hold its line rate on
a table of the row table's size?  A row table for config 3 is 4^13 rows of 1 KiB = 64 GiB, eight times config 3's own 8 GiB table; a
far larger allocation may lose line rate to address translation.  Both tables are created in this process (zeroed, never filled: the
probe attaches no compute and never looks at the bits), each one is probed with 1 KiB rows, non-temporal loads on and off, 12 and 24
loads in flight per wave, the two tables alternated, `repeats` times; the figure of a setting is its best run, as bench.py reads the
probe.  Break-even for one gather per k-mer in place of three is the model's line ratio, 4 871 / 12 904 = 0.38.

  python3 profiles/row_table_probe.py [repeats, default 3] [log2 of the large table's rows, default 26 = 4^13]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from readbouncer_amd import capi  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
lg_rows = int(sys.argv[2]) if len(sys.argv) > 2 else 26
N_BINS, K, H, ROW = 8192, 13, 3, 1024
BREAK_EVEN = 4871.0 / 12904.0

capi.set_placement_tries(1)  # one allocation each: the question is the size, not which of five candidates is the fast kind
tables = {}
for name, rows in (("c3_8GiB", 1 << 23), ("rows_%dGiB" % ((ROW << lg_rows) >> 30), 1 << lg_rows)):
    t0 = time.perf_counter()
    d = capi.DeviceIBF.create(0, N_BINS, H, K, N_BINS * rows)
    assert d.info["n_blocks"] == rows and capi.lib().rb_dibf_device_stride(d.h) * 8 == ROW, d.info
    tables[name] = (d, rows, time.perf_counter() - t0)
    print("%s: %d rows of %d bytes, created and zeroed in %.2f s" % (name, rows, ROW, tables[name][2]), flush=True)

SETTINGS = [(nt, lif) for nt in (1, 0) for lif in (12, 24)]
runs = {name: {s: [] for s in SETTINGS} for name in tables}
for rep in range(reps + 1):  # the first round warms up (clocks, code object) and is not counted
    for name in (list(tables)[::-1] if rep % 2 else list(tables)):
        for s in SETTINGS:
            gbps, ms = tables[name][0].probe_read_peak(ROW, s[0], s[1], target_ms=150.0)
            if rep:
                runs[name][s].append(gbps)
            print("rep %d %-12s nt=%d in_flight=%2d  %8.1f GB/s  %6.2f G lines/s  (%.0f ms)" % (rep, name, s[0], s[1], gbps, gbps / 128.0, ms),
                  flush=True)

small, large = list(tables)
res = {"row_bytes": ROW, "repeats": reps, "break_even_ratio": round(BREAK_EVEN, 4), "tables": {}, "ratio_large_to_small": {}}
for name in tables:
    res["tables"][name] = {"rows": tables[name][1], "bytes": tables[name][1] * ROW, "create_s": round(tables[name][2], 3),
                           "gbps": {"nt%d_b%d" % s: round(max(v), 1) for s, v in runs[name].items()},
                           "glines_per_s": {"nt%d_b%d" % s: round(max(v) / 128.0, 2) for s, v in runs[name].items()},
                           "spread": {"nt%d_b%d" % s: round((max(v) - min(v)) / max(v), 4) for s, v in runs[name].items()}}
for s in SETTINGS:
    res["ratio_large_to_small"]["nt%d_b%d" % s] = round(max(runs[large][s]) / max(runs[small][s]), 4)
best = {name: max(max(v) for v in runs[name].values()) for name in tables}
res["ratio_best_to_best"] = round(best[large] / best[small], 4)
res["go_on"] = res["ratio_best_to_best"] > BREAK_EVEN
print(json.dumps(res))
