#!/usr/bin/env python3
"""CPU model of the plain count kernel's fabric lines per read under bound pruning (rb_kernels.hip, count_strand), numpy only.

The filter is config 3's: 8192 bins = 64 lanes of 128 bins (16 bytes) = 8 lines of 128 bytes per block, three hashes, random fill at
rbspec::synth_word's bit density (55/256 per bit).  A read is 360 bp = 348 13-mers.  Read kinds follow synth.make_reads: negatives
(uniform), positives at 10 % nominal substitutions (a quarter restore the base: 7.5 % effective), a tenth of the positives at
19-23 % nominal, every second positive given as its reverse complement.  Per k-mer and bin a chance hit is Bernoulli(d) for hash 0
and Bernoulli(d^2) more for the other two; a planted k-mer (no error in its 13 bases) hits its bin on its strand.

What is counted: per k-mer step, h (3, or 1 in a certificate pass) times the 128-byte lines that still have a live lane.  A lane is
live while one of its bins has count > M - rem; M is the best count the wave holds (fresh at a tile boundary, stale in between).
Dead lanes read block 0, which never leaves the cache.

States: no pruning; today (checks at 64-k-mer tile boundaries, forward strand first); and the combinations of
  part 1  a check after every 8 k-mers (M stale since the tile boundary),
  part 2  both strands probed for 64 k-mers, the one with the larger probe maximum finished first (tie: forward),
  part 3  the trailing strand certified from hash 0 alone when the leader's maximum is at least
          probe maximum + ceil(d rem + z sqrt(d (1 - d) rem)), z = 4.5.  (The kernel also prunes inside that pass and leaves it at the
          first counter above the leader's maximum; the model gathers it with the lanes alive on entry, so it reads a little high there.)
  part 4  the lead line (needs parts 2 and 3): when the leader's probe maximum is at least LEAD_MIN, the 8 lanes of the 128-byte line that
          holds its best probe bin are counted first, alone, from k-mer 64 (3 lines per k-mer); the other 56 lanes are then certified from
          hash 0 against the line's maximum by the rule of part 3 (pruned and left early as in the kernel), counted in full from k-mer 64
          against it where the rule is not met, or counted again from k-mer 0 where the certificate fails.
  rows_line  the rows state with the lead line on top (a model only: the kernel has no such build).
  rows    the row form (ibf_count_rows_kernel): one gather per k-mer from the filter's row table, whose row is the AND of the k-mer's three
          blocks -- the counts are the full counts, every step costs one line per live line instead of three -- under parts 1 and 2;
          hash 0 alone being the whole count, parts 3 and 4 have nothing to certify.
  lists   the list form (ibf_count_lists_kernel): one slot of LIST_LINES lines per k-mer from the filter's list table, a counter per bin
          in LDS.  No lane dies (a slot is fetched whole or not at all): the forward strand is counted to its end, the reverse strand is
          skipped when the forward one reached N and stops at the first tile boundary where its maximum so far plus the k-mers to come
          cannot pass the forward maximum.
  lists_lead  the lists state with the strand lead on top (a model only: it needs a second counter array or a recount of the loser's
          probe): both strands probed for 64 k-mers, the stronger finished first, the other continued against its maximum.

  python3 profiles/prune_model.py [reads per kind, default 500] [seed, default 1]
  python3 profiles/prune_model.py --calibrate [reads per kind, default 4000] [seed, default 1]
      today's state alone, checked against its measurement: the gate of every prediction above.  A pass without sub-tile checks looks at
      the counters at tile boundaries only, so this run draws each bin's hits of a whole tile at once (Binomial(64, d^3): the same
      distribution as 64 draws per k-mer) and goes through the same read_lines / run_strand -- a hundredth of the random numbers.
"""
import math
import sys

import numpy as np

N, TILE, LANES, BPL, LPL, H = 348, 64, 64, 128, 8, 3  # k-mers, tile, lanes, bins per lane, lanes per line, hashes
D = 55.0 / 256.0
Z = 4.5
LIST_LINES = 2  # lines per slot of the list table at this load: 81 of 8192 bins per row, 128 entries
LEAD_MIN = 8  # probe maxima of reads without a match stay below it
MEASURED_TODAY = 15698.1  # TCC_EA0_RDREQ per read, profiles/bound_pruning/bench_ab.txt


def strand_counts(rng, planted):
    """per-bin cumulative counts of one strand, all hashes and hash 0 alone: two arrays [N + 1][bins]; planted = bool[N] or None"""
    h0 = rng.random((N, LANES * BPL), dtype=np.float32) < D
    full = h0 & (rng.random((N, LANES * BPL), dtype=np.float32) < D * D)
    if planted is not None:
        b = int(rng.integers(0, LANES * BPL))
        full[:, b] |= planted
        h0[:, b] |= planted
    out = []
    for hits in (full, h0):
        c = np.zeros((N + 1, LANES * BPL), dtype=np.int32)
        np.cumsum(hits, axis=0, out=c[1:])
        out.append(c)
    return out  # per-bin cumulative counts (full, hash 0)


class TileCounts:
    """per-bin cumulative counts at the tile boundaries and at N alone: all that a pass without sub-tile checks looks at"""

    def __init__(self, rows):
        self.rows = rows  # [tiles + 1][bins]; rows[0] = 0, rows[-1] = the counts at N

    def __getitem__(self, q):
        assert q == N or q % TILE == 0, q
        return self.rows[-1] if q == N else self.rows[q // TILE]


def tile_counts(rng, planted):
    """strand_counts' all-hash counts in distribution, drawn tile by tile; planted = bool[N] or None"""
    edges = list(range(0, N, TILE)) + [N]
    sizes = np.diff(edges)
    hits = np.stack([rng.binomial(int(n), D ** 3, size=LANES * BPL) for n in sizes]).astype(np.int32)
    if planted is not None:
        b = int(rng.integers(0, LANES * BPL))
        col = (rng.random(N) < D ** 3) | planted
        hits[:, b] = [int(col[lo:hi].sum()) for lo, hi in zip(edges[:-1], edges[1:])]
    rows = np.zeros((len(sizes) + 1, LANES * BPL), dtype=np.int32)
    np.cumsum(hits, axis=0, out=rows[1:])
    return TileCounts(rows)


def lines_of(live):
    return int(live.reshape(LANES // LPL, LPL).any(axis=1).sum())


def run_strand(c, start, bb, sub, lanes=None, h=H, off=None, stop_above=None):
    """pass over k-mers [start, N) with bound bb and h hashes; returns (lines, held maximum).  c = per-bin cumulative counts.
    lanes: the lanes that take part (default all); the others hold `off` (default: their counts at `start`) throughout.
    stop_above: a certificate pass, left at the first tile boundary that sees a counter above it"""
    lanes_of_bin = np.repeat(np.arange(LANES), BPL)
    live = np.ones(LANES, dtype=bool) if lanes is None else lanes.copy()
    held = np.zeros(LANES * BPL, dtype=np.int32)  # counters of dead lanes, frozen
    if lanes is not None:
        out = ~lanes[lanes_of_bin]
        held[out] = (c[start] if off is None else off)[out]
    lines, pos, m_stale = 0, start, bb

    def check(q, m):
        nonlocal live, held
        rem = N - q
        if m < rem:
            return
        cur = c[q]
        alive_bin = cur > (m - rem)
        lane_alive = alive_bin.reshape(LANES, BPL).any(axis=1)
        dying = live & ~lane_alive
        if dying.any():
            sel = dying[lanes_of_bin]
            held[sel] = cur[sel]
            live &= lane_alive

    def held_max(q):
        cur = np.where(live[lanes_of_bin], c[q], held)
        return int(cur.max())

    if start > 0:  # entry check at the probe's end
        m_stale = max(bb, held_max(start))
        check(start, m_stale)
    while pos < N and live.any():
        nxt = min(N, (pos // TILE + 1) * TILE)
        if sub:
            nxt = min(nxt, pos + 8)
        lines += h * lines_of(live) * (nxt - pos)
        pos = nxt
        if pos >= N:
            break
        if pos % TILE == 0:
            m_stale = max(bb, held_max(pos))
            if stop_above is not None and m_stale > stop_above:
                break
            check(pos, m_stale)
        else:
            check(pos, m_stale)
    return lines, held_max(min(pos, N))


def list_strand_rows(c, start, best):
    """slots gathered by the list kernel over k-mers [start, N) of a strand with cumulative counts c, against `best` (0: no bound)"""
    for q in range((start // TILE) * TILE, N, TILE):
        if q >= start and q > 0 and best and int(c[q].max()) + (N - q) <= best:
            return q - start
    return N - start


def allowance(rem):
    return math.ceil(D * rem + Z * math.sqrt(D * (1 - D) * rem))


def lead_line(c, c0, sub):
    """part 4 on the leader strand (c: all hashes, c0: hash 0, cumulative): (lines behind the probe, maximum, certificate tried, held), or
    None where the probe maximum is below LEAD_MIN"""
    probe = c[TILE]
    if int(probe.max()) < LEAD_MIN:
        return None
    line = int(np.argmax(probe)) // BPL // LPL  # (the first bin with the maximum: the lowest lane)
    mine = np.arange(LANES) // LPL == line
    rem = N - TILE
    l1, m_line = run_strand(c, TILE, 0, sub, lanes=mine)
    others = ~mine
    theirs = int(probe[np.repeat(others, BPL)].max())
    zeros = np.zeros(LANES * BPL, dtype=np.int32)  # (the line's lanes are finished: the bound carries their maximum)
    if m_line >= theirs + allowance(rem):
        ub = probe[None, :] + (c0 - c0[TILE][None, :])
        l2, m2 = run_strand(ub, TILE, m_line, sub, lanes=others, h=1, off=zeros, stop_above=m_line)
        if m2 <= m_line:
            return l1 + l2, m_line, 1, 1
        l3, m3 = run_strand(c, 0, m_line, sub, lanes=others, off=zeros)
        return l1 + l2 + l3, max(m_line, m3), 1, 0
    l3, m3 = run_strand(c, TILE, m_line, sub, lanes=others, off=zeros)
    return l1 + l3, max(m_line, m3), 0, 0


def read_lines(rng, kind, only_today=False):
    """lines per read under every state for one read of `kind` = (planted strand or None, effective error rate); only_today: the states
    without pruning and with today's alone, from counts drawn per tile (tile_counts)"""
    strand, e = kind
    planted = None
    if strand is not None:
        err = rng.random(N + 12) < e
        bad = np.convolve(err.astype(np.int32), np.ones(13, dtype=np.int32), mode="valid") > 0
        planted = ~bad
    if only_today:
        cs = [[tile_counts(rng, planted if strand == s else None)] for s in (0, 1)]
    else:
        cs = [strand_counts(rng, planted if strand == s else None) for s in (0, 1)]
    res = {"none": 2 * N * H * (LANES // LPL)}
    for sub in ((0,) if only_today else (0, 1)):  # forward first (today, and part 1 alone)
        l0, m0 = run_strand(cs[0][0], 0, 0, sub)
        l1, m1 = (0, 0) if m0 >= N else run_strand(cs[1][0], 0, m0, sub)
        res["today" if not sub else "1"] = l0 + l1
        assert max(m0, m1) == max(int(cs[0][0][N].max()), int(cs[1][0][N].max()))
    if only_today:
        return res
    probe = 2 * TILE * H * (LANES // LPL)
    p = [int(cs[s][0][TILE].max()) for s in (0, 1)]
    lead = 1 if p[1] > p[0] else 0
    trail = lead ^ 1
    for sub in (0, 1):
        ll, m = run_strand(cs[lead][0], TILE, 0, sub)
        lt, mt = (0, 0) if m >= N else run_strand(cs[trail][0], TILE, m, sub)
        res["2" if not sub else "12"] = probe + ll + lt
        if sub:  # the same passes with one gather per k-mer
            rl, rm = run_strand(cs[lead][0], TILE, 0, sub, h=1)
            rt, rmt = (0, 0) if rm >= N else run_strand(cs[trail][0], TILE, rm, sub, h=1)
            assert (rm, rmt) == (m, mt)
            res["rows"] = probe // H + rl + rt
            # ... and the lead line on top of it (not built): the leader's best probe line first, alone, then its other lanes in full
            # against that line's maximum -- one gather per k-mer throughout, nothing to certify
            res["rows_line"] = res["rows"]
            lead_probe = cs[lead][0][TILE]
            if int(lead_probe.max()) >= LEAD_MIN:
                mine = np.arange(LANES) // LPL == int(np.argmax(lead_probe)) // BPL // LPL
                l1, m_line = run_strand(cs[lead][0], TILE, 0, sub, lanes=mine, h=1)
                l3, m3 = run_strand(cs[lead][0], TILE, m_line, sub, lanes=~mine, off=np.zeros(LANES * BPL, dtype=np.int32), h=1)
                assert max(m_line, m3) == m
                lt2, mt2 = (0, 0) if m >= N else run_strand(cs[trail][0], TILE, m, sub, h=1)
                res["rows_line"] = probe // H + l1 + l3 + lt2
            # the list form: whole slots, the forward strand first and unbounded
            f_max, r_max = int(cs[0][0][N].max()), int(cs[1][0][N].max())
            res["lists"] = LIST_LINES * (N + (0 if f_max >= N else list_strand_rows(cs[1][0], 0, f_max)))
            lead_max = int(cs[lead][0][N].max())
            res["lists_lead"] = LIST_LINES * (2 * TILE + (N - TILE) + (0 if lead_max >= N else list_strand_rows(cs[trail][0], TILE, lead_max)))
        assert max(m, mt) == max(int(cs[0][0][N].max()), int(cs[1][0][N].max()))
        # part 3: hash 0 alone over [TILE, N) on top of the trailing probe's counters
        rem = N - TILE
        tot = probe + ll + lt
        tried = held = False
        if m < N and m >= p[trail] + allowance(rem):
            tried = True
            ub = cs[trail][0][TILE] + (cs[trail][1][N] - cs[trail][1][TILE])
            # lanes that the entry check kills are not gathered in the certificate pass either
            live = (cs[trail][0][TILE] > (m - rem)).reshape(LANES, BPL).any(axis=1) if m >= rem else np.ones(LANES, dtype=bool)
            cert = lines_of(live) * rem
            ub_max = int(np.where(np.repeat(live, BPL), ub, 0).max())
            held = ub_max <= m
            tot = probe + ll + cert + (0 if held else lt)
        res["23" if not sub else "123"] = tot
        res["cert_tried"], res["cert_held"] = int(tried), int(held)
        if sub:  # part 4 on top of 1-3: the leader by its line, the trailing strand as before against the same maximum
            got = lead_line(cs[lead][0], cs[lead][1], sub)
            res["line_tried"], res["line_cert"], res["line_held"] = int(got is not None), 0, 0
            res["1234"] = tot
            res["true_max"] = res["max_1234"] = max(m, mt)
            if got is not None:
                l4, m4, res["line_cert"], res["line_held"] = got
                assert m4 == m, (m4, m)  # the leader's maximum is exact whichever way it was found
                res["1234"] = tot - ll + l4
                res["max_1234"] = max(m4, mt)
    return res


KINDS = {"neg": (None, 0.0), "pos_fwd": (0, 0.075), "pos_rev": (1, 0.075), "near_fwd": (0, None), "near_rev": (1, None)}
GATE = 0.002  # today's state within 0.2 % of its measurement, or no prediction is quoted


def bench_mix(means, k):
    pos = 0.45 * (means["pos_fwd"][k] + means["pos_rev"][k]) + 0.05 * (means["near_fwd"][k] + means["near_rev"][k])
    return 0.5 * means["neg"][k] + 0.5 * pos


def calibration(per_kind=4000, seed=1):
    """today's state on the bench mix from per-tile draws -> (model lines per read, relative distance from MEASURED_TODAY)"""
    rng = np.random.default_rng(seed)
    means = {}
    for name, (strand, e) in KINDS.items():
        tot = 0
        for _ in range(per_kind):
            tot += read_lines(rng, (strand, e if e is not None else 0.75 * rng.uniform(0.19, 0.23)), only_today=True)["today"]
        means[name] = {"today": tot / per_kind}
    today = bench_mix(means, "today")
    return today, today / MEASURED_TODAY - 1.0


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--calibrate":
        per_kind = int(sys.argv[2]) if len(sys.argv) > 2 else 4000
        today, off = calibration(per_kind, int(sys.argv[3]) if len(sys.argv) > 3 else 1)
        print("today's state on the bench mix, %d reads per kind: model %.0f, measured %.1f (%+.2f %%)" % (per_kind, today, MEASURED_TODAY, 100 * off))
        return 0 if abs(off) <= GATE else 1
    per_kind = int(sys.argv[1]) if len(sys.argv) > 1 else 500
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    rng = np.random.default_rng(seed)
    kinds = KINDS
    means = {}
    for name, (strand, e) in kinds.items():
        acc = {}
        for _ in range(per_kind):
            ee = e if e is not None else 0.75 * rng.uniform(0.19, 0.23)
            for k, v in read_lines(rng, (strand, ee)).items():
                acc[k] = acc.get(k, 0) + v
        means[name] = {k: v / per_kind for k, v in acc.items()}
        print(name, {k: round(v, 1) for k, v in means[name].items()}, flush=True)
    pos = {k: 0.45 * (means["pos_fwd"][k] + means["pos_rev"][k]) + 0.05 * (means["near_fwd"][k] + means["near_rev"][k]) for k in means["neg"]}
    mixes = {"bench": {k: 0.5 * means["neg"][k] + 0.5 * pos[k] for k in pos}, "positive": pos, "negative": means["neg"]}
    print("\nfabric lines per read (model, %d reads per kind, seed %d)" % (per_kind, seed))
    states = ("none", "today", "1", "2", "12", "23", "123", "1234", "rows", "rows_line", "lists", "lists_lead")
    print("%-10s" % "mix" + "".join("%11s" % ("parts " + s if s[0].isdigit() else s) for s in states) + "  cert tried/held  line tried/cert/held")
    for mix, v in mixes.items():
        print("%-10s" % mix + "".join("%11.0f" % v[s] for s in states) + "  %.3f / %.3f  %.3f / %.3f / %.3f" % (
            v["cert_tried"], v["cert_held"], v["line_tried"], v["line_cert"], v["line_held"]))
    today = mixes["bench"]["today"]
    off = today / MEASURED_TODAY - 1.0
    print("\ntoday's state on the bench mix: model %.0f, measured %.1f (%+.2f %%)" % (today, MEASURED_TODAY, 100 * off))
    if abs(off) > GATE:
        print("MODEL NOT CALIBRATED: today's state is more than 0.2 % off the measurement; do not quote the predictions")
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
