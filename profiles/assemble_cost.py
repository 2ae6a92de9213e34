"""What assembling a filter from bins of a resident one costs, beside what the box streams.

  c3            config 3's filter (8 GiB, 8 192 bins, W = 128)
  grch38_f100k  GRCh38 at fragment_size 100 000 (31 000 bins, W = 485, stride 496)

Per shape, on a filter under the synthetic fill, in one run:
  identity      out bin j = bin j                              (reads the table once, writes it once)
  reversed      out bin j = bin n - 1 - j                      (the same traffic, every lane a different source word)
  merge8        out bin j = bins [8 j, 8 j + 8)                (reads the table, writes an eighth)
  scattered     a random permutation of the bins: every tile of 4 096 out bins names the whole source block, so the block is staged
                once per tile (twice on config 3, eight times on GRCh38-F100k) -- the weak spot DESIGN 4.9 names
  join          two halves of the bins, made by select_bins, joined back into one table (two sources)
  resize        rb_dibf_resize_bins to the same bin count: the restride kernel, the identity's traffic
  probe         DeviceIBF.probe_read_peak with rows of one block, the project's "what the box delivers"
Times: the assemble kernel alone (rb_assemble_last_seconds: a hipEvent pair around the launch) and the wall time of the whole call; for
resize the wall time of the call (allocation, an 8 GiB memset of the new table and the restride kernel -- the library does not time that
kernel by itself), so the like-for-like ratio is wall against wall and the kernel figure stands beside it.  Placement by trial is
switched off for the run (rb_set_placement_tries(1)): it would add seconds of probing to every call's wall time.  The yardstick of the
merge is the probe's time for the bytes it moves.  Nothing here asserts a time; the identity's result is compared with its source
(rb_dibf_compare) before anything is timed.

Method (measuring guide): one warm-up of every leg, then REPS repetitions with the legs ALTERNATED (identity, reversed, merge8, join,
resize, probe, identity, ...), medians, the spread (min-max) stated.
usage: python profiles/assemble_cost.py [--legs c3,grch38_f100k] [--reps 5] [--out profiles/assemble/cost.txt]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from readbouncer_amd import capi, synth  # noqa: E402


def run_leg(name, reps, say):
    w = synth.WORKLOADS[name]
    dev = capi.DeviceIBF.create(0, w["n_bins"], w["h"], w["k"], synth.filter_bits(w))
    dev.fill_synth(9)
    info, stride = dev.info, dev.device_stride()
    n = info["n_bins"]
    table = info["n_blocks"] * stride * 8
    nt = table > capi.nt_threshold_default()
    row = 4096 if stride * 8 >= 3072 else 1024 if stride * 8 >= 1024 else 128
    half = n // 2
    lo, hi = dev.select_bins(range(half)), dev.select_bins(range(half, n))
    plans = {
        "identity": ([dev], capi.assemble_plan([[(0, b)] for b in range(n)])),
        "reversed": ([dev], capi.assemble_plan([[(0, n - 1 - b)] for b in range(n)])),
        "scattered": ([dev], capi.assemble_plan([[(0, int(b))] for b in np.random.default_rng(3).permutation(n)])),
        "merge8": ([dev], capi.assemble_plan([[(0, b) for b in range(j, min(j + 8, n))] for j in range(0, n, 8)])),
        "join": ([lo, hi], capi.assemble_plan([[(0, b)] for b in range(half)] + [[(1, b)] for b in range(n - half)])),
    }

    def assemble(key):
        srcs, plan = plans[key]
        t0 = time.perf_counter()
        out = capi.DeviceIBF.assemble(srcs, plan)
        wall = time.perf_counter() - t0
        return out, capi.assemble_last_seconds() * 1e3, wall * 1e3

    def resize():
        t0 = time.perf_counter()
        out = dev.resize_bins(n)
        wall = (time.perf_counter() - t0) * 1e3
        out.free()
        return wall

    def probe():
        return dev.probe_read_peak(row, nt, 24, target_ms=60.0)[0]

    # warm-up, and the identity and the join against their source before anything is timed
    for key in plans:
        out, _, _ = assemble(key)
        if key in ("identity", "join"):
            c = dev.compare(out)
            assert c["file_bits"] == c["rebuilt_bits"] and c["new_bits"] == 0, (key, c)
            c = out.compare(dev)
            assert c["new_bits"] == 0, (key, c)
        out.free()
    resize(), probe()
    kern = {k: [] for k in plans}
    wall = {k: [] for k in plans}
    rs, gb = [], []
    for _ in range(reps):  # alternated
        for key in plans:
            out, k_ms, w_ms = assemble(key)
            out.free()
            kern[key].append(k_ms)
            wall[key].append(w_ms)
        rs.append(resize())
        gb.append(probe())
    say("%s: %d bins, W = %d words, stride %d, %d blocks, table %.1f MiB (%s), %d alternated repetitions"
        % (name, n, info["bin_width"], stride, info["n_blocks"], table / 2**20, "non-temporal" if nt else "cached", reps))
    med = statistics.median
    for key in plans:
        say("  %-9s kernel: median %9.3f ms (min %.3f, max %.3f)   call: median %9.3f ms (min %.3f, max %.3f)"
            % (key, med(kern[key]), min(kern[key]), max(kern[key]), med(wall[key]), min(wall[key]), max(wall[key])))
    say("  resize    call  : median %9.3f ms (min %.3f, max %.3f)" % (med(rs), min(rs), max(rs)))
    g = med(gb)
    say("  probe, rows of %4d B: median %.0f GB/s (min %.0f, max %.0f)" % (row, g, min(gb), max(gb)))
    moved = table + info["n_blocks"] * ((-(-n // 8) + 63) // 64) * 8  # the source, and the merged table's payload
    floor = moved / (g * 1e9) * 1e3
    say("  identity / resize (call against call)  : %.2f     identity kernel / resize call: %.2f"
        % (med(wall["identity"]) / med(rs), med(kern["identity"]) / med(rs)))
    say("  reversed / resize (call against call)  : %.2f     reversed kernel / resize call: %.2f"
        % (med(wall["reversed"]) / med(rs), med(kern["reversed"]) / med(rs)))
    say("  scattered/ resize (call against call)  : %.2f     scattered kernel / resize call: %.2f"
        % (med(wall["scattered"]) / med(rs), med(kern["scattered"]) / med(rs)))
    say("  join     / resize (call against call)  : %.2f     join kernel / resize call    : %.2f"
        % (med(wall["join"]) / med(rs), med(kern["join"]) / med(rs)))
    say("  merge8 kernel / probe's time for the %.2f GiB it moves (%.3f ms): %.2f" % (moved / 2**30, floor, med(kern["merge8"]) / floor))
    for f in (lo, hi, dev):
        f.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="c3,grch38_f100k")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assemble", "cost.txt"))
    args = ap.parse_args()
    assert args.reps >= 5, "at least five alternated repetitions"
    if capi.device_count() <= 0:
        sys.exit("assemble_cost.py needs a GPU")
    capi.set_placement_tries(1)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        def say(line):
            print(line, flush=True)
            fh.write(line + "\n")
            fh.flush()
        say("assemble cost -- library %s" % os.path.basename(capi.LIB_PATH))
        for leg in args.legs.split(","):
            run_leg(leg.strip(), args.reps, say)


if __name__ == "__main__":
    main()
