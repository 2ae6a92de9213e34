"""What the per-bin occupancy pass costs: ms per pass over a resident filter, beside what the box streams.

  c3            config 3's filter (8 GiB, W = 128)
  grch38_f100k  GRCh38 at fragment_size 100 000 (W = 485, stride 496)
  c2            config 2's filter (W = 16)
  mock_deplete, mock_t1   the README shape's narrow filters (W = 2, W = 1)

Per shape: the pass (rb_dibf_bin_occupancy_device into a device buffer, hipEvent pair around the call on one stream: the memset of the
output and the kernel) and, ALTERNATED with it in the same run, the box's streaming figure -- DeviceIBF.probe_read_peak with rows the
size of one block (128, 1024 or 4096 bytes, whichever is next) on the same table, the project's "what the box delivers".  Beside each time: payload bytes (n_blocks * W * 8) / time, the
probe's GB/s, and their ratio.  Expectation: the pass does about one carry-save step per loaded word and should run at the probe's
rate; a ratio below 0.8 on the 8 GiB table wants counters (rocprofv3 --kernel-trace --stats for the time, --pmc TCC_EA0_RDREQ in a run
of its own), not blind tuning.  Nothing here asserts a time.

Method (measuring guide): one warm-up pair, then REPS alternated repetitions (pass, probe, pass, probe, ...), medians, the spread
(min-max) stated.  usage: python profiles/filter_stats_cost.py [--legs c3,grch38_f100k,c2,mock_deplete,mock_t1] [--reps 7]
[--out profiles/filter_stats/cost.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from readbouncer_amd import capi, synth  # noqa: E402


def run_leg(name, reps, torch, say):
    w = synth.WORKLOADS[name]
    dev = capi.DeviceIBF.create(0, w["n_bins"], w["h"], w["k"], synth.filter_bits(w))
    dev.fill_synth(9)
    info, stride = dev.info, dev.device_stride()
    payload = info["n_blocks"] * info["bin_width"] * 8
    table = info["n_blocks"] * stride * 8
    nt = table > capi.nt_threshold_default()  # the library's own rule for the pass; the probe reads the same way
    out = torch.zeros(info["n_bins"], dtype=torch.int64, device="cuda:0")
    stream = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()

    def one_pass():
        with torch.cuda.stream(stream):
            e0.record(stream)
            dev.bin_occupancy_device(out.data_ptr(), stream.cuda_stream)
            e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1)

    # the probe gathers rows of 128, 1024 or 4096 bytes: the size next to one block, by the rule of the library's placement trial
    row = 4096 if stride * 8 >= 3072 else 1024 if stride * 8 >= 1024 else 128

    def probe():
        return dev.probe_read_peak(row, nt, 24, target_ms=60.0)[0]

    one_pass(), probe()  # warm-up
    total = int(out.sum().item())
    assert total == dev.compare(dev)["file_bits"], "the pass and the comparison kernel disagree on the number of set bits"
    ms, gbps = [], []
    for _ in range(reps):  # alternated
        ms.append(one_pass())
        gbps.append(probe())
    m, g = statistics.median(ms), statistics.median(gbps)
    rate = payload / (m * 1e-3) / 1e9
    say("%s: %d bins, W = %d words, stride %d, %d blocks, payload %.1f MiB (table %.1f MiB, %s loads), %d alternated repetitions"
        % (name, info["n_bins"], info["bin_width"], stride, info["n_blocks"], payload / 2**20, table / 2**20, "non-temporal" if nt else "cached", reps))
    say("  pass                 : median %.4f ms  (min %.4f, max %.4f)" % (m, min(ms), max(ms)))
    say("  payload / time       : %.0f GB/s" % rate)
    say("  probe, rows of %4d B: median %.0f GB/s  (min %.0f, max %.0f)" % (row, g, min(gbps), max(gbps)))
    say("  pass / probe         : %.3f" % (rate / g))
    dev.free()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="c3,grch38_f100k,c2,mock_deplete,mock_t1")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter_stats", "cost.txt"))
    args = ap.parse_args()
    assert args.reps >= 5, "at least five alternated repetitions"
    import torch
    if capi.device_count() <= 0:
        sys.exit("filter_stats_cost.py needs a GPU")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        def say(line):
            print(line, flush=True)
            fh.write(line + "\n")
            fh.flush()
        say("filter-stats cost -- %s, library %s" % (torch.cuda.get_device_name(0), os.path.basename(capi.LIB_PATH)))
        for leg in args.legs.split(","):
            run_leg(leg.strip(), args.reps, torch, say)


if __name__ == "__main__":
    main()
