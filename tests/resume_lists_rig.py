"""Fixtures of tests/test_gpu_resume_lists.py: the list form of the resume pass (rb_resume_lists.hip) counts a feed's new k-mers into
16-bit LDS counters and merges them into the slot's bit-sliced planes, lane l at the columns l, l + 64, ... of 64 bins.  The schedules
here feed chunks below k, across the seam between two chunks, empty ones, a full tile and a part tile; walk a slot's totals across the
uint16_t wrap in feeds that each stay below 65 536 k-mers; and mix the kinds of item the list kernel takes and leaves.  Host arithmetic
only: tests/test_resume_lists_cpu.py asserts on the oracle alone that the fixtures are what they claim."""
from tests import list_scan_rig as SR
from tests import pass_edges as PE
from tests import pass_lists_edges_rig as ER
from tests import resume_rules as RR

K = SR.K
rc = SR.rc
ACGT = set("ACGT")


# ------------------------------------------------------------------------------------------------ the schedule of every geometry
def schedule(k):
    """chunk lengths: below k, one base at a time across the seam, an empty chunk, a few bases, a full tile and a part tile (70 k-mers),
    then short ones again and three tiles and a part"""
    return (k - 1, 1, 1, 0, 5, 70, 3, k - 2, 200)


COUNT_CHECKS = (0, 4, 5, 8)  # after the feeds to k - 1 bases, of 5, of 70 and the last one
MAX_CHUNK = 200
MAX_TOTAL = sum(schedule(K))


def schedule_reads(f):
    """SR.Planted's reads and their reverse complements (the shorter ones run out: empty chunks from then on), and three reads that
    last the whole schedule, with their reverse complements"""
    long = [f.plants[-1] + f.plants[-2], f.plants[-3] + f.plants[-4], f.plants[-5] + f.plants[-6]]
    return f.reads() + long + [rc(r) for r in long]


# ------------------------------------------------------------------------------------------------ the wrap
WRAP_GEOMETRIES = ((8192, 2), ER.ODD)
WRAP_TOTALS = (32767, 65534, 65535, 65536, 65537, 70000)  # a slot's k-mers after successive feeds
WRAP_SAT = (32767, 65534, 65535, 0, 1, 4464)              # ... and what a bin set in every block then holds
WRAP_MAX_TOTAL = 70100


def wrap_ends(k):
    return tuple(n + k - 1 for n in WRAP_TOTALS)


def wrap_reads(k):
    s = PE.sequence()[:WRAP_TOTALS[-1] + k - 1]
    return [s, rc(s)]


# ------------------------------------------------------------------------------------------------ who takes which item
def taken_items(model, items, k, bad_chunk=()):
    """which items of a feed the list kernel takes, BEFORE the model commits it: not refused, and "tail + chunk" holds no base outside
    ACGT (any length)"""
    out = []
    for i, (slot, chunk, flags) in enumerate(items):
        concat = None if i in bad_chunk else model.verdict(slot, chunk, flags)[1]
        if concat is None:
            out.append(False)
            continue
        seen = "" if flags & RR.FIRST else model.seen.get(slot, "")
        out.append(set(RR.stitched(seen, chunk, k)) <= ACGT)
    return out


MIX_KINDS = ("free", "n_first", "free", "n_last", "free", "n_mid", "free", "bad_slot", "free", "too_long", "free", "short")
MIX_SLOTS = len(MIX_KINDS)
MIX_MAX_CHUNK = 120
MIX_FIRST, MIX_SECOND, MIX_THIRD = 100, 60, 50  # bases of the three feeds


def mixed_feeds(f):
    """-> (first, second, third, kinds): three feeds of one item per slot.  First (FIRST everywhere): N-free chunks interleaved with an
    N in the chunk's first, last and a middle base (the second tile), a slot number beyond the set, a chunk longer than max_chunk_len
    and a chunk of k - 2 bases.  Second and third: N-free chunks everywhere (the two refused items stay refused) -- in the second the
    slot fed "....N" still has the N in its tail, in the third no longer."""
    kinds = list(MIX_KINDS)
    reads = schedule_reads(f)[-6:] * 2  # twelve reads of 322 bases and more
    feeds = []
    for step, (lo, n) in enumerate(((0, MIX_FIRST), (MIX_FIRST, MIX_SECOND), (MIX_FIRST + MIX_SECOND, MIX_THIRD))):
        items = []
        for s, (kind, r) in enumerate(zip(kinds, reads)):
            chunk, slot = r[lo:lo + n], s
            if kind == "bad_slot":
                slot = MIX_SLOTS + 5
            elif kind == "too_long":
                chunk = r[:MIX_MAX_CHUNK + 1]
            elif step == 0:
                if kind == "n_first":
                    chunk = "N" + chunk[1:]
                elif kind == "n_last":
                    chunk = chunk[:-1] + "N"
                elif kind == "n_mid":
                    chunk = chunk[:70] + "N" + chunk[71:]
                elif kind == "short":
                    chunk = chunk[:K - 2]
            items.append((slot, chunk, RR.FIRST if step == 0 else 0))
        feeds.append(items)
    return feeds[0], feeds[1], feeds[2], kinds
