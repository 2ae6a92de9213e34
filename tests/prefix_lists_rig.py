"""Fixtures of tests/test_gpu_prefix_lists.py: the list form of the prefix pass (rb_prefix_lists.hip) counts the k-mers between two
checkpoints from a filter's list table -- a range that begins wherever the last checkpoint ended, inside a 64-k-mer tile or a batch of
slots as often as at their seams -- scans the 16-bit counters after every checkpoint that adds a k-mer, keeps checkpoint p's maximum
over the two strands in lane p, and takes the items whose first min(length, last checkpoint) bases are all ACGT.  The fixtures put
checkpoints one k-mer apart across those seams, move the maximum between strands and bins from one checkpoint to the next, and mix the
kinds of item the kernel takes and leaves; takes() is the rule itself, written from the header's words.  Host arithmetic on the
oracle's words only: the GPU tests upload the same words, and tests/test_prefix_lists_cpu.py asserts on the oracle alone that the
fixtures are what they claim."""
import numpy as np

from oracle import pyoracle as po
from tests import helpers as H
from tests import list_scan_rig as SR
from tests import pass_edges as PE
from tests import pass_lists_edges_rig as ER
from tests import pass_lists_rig as PL

K = SR.K
R, CONF = PL.R, PL.CONF
rc = SR.rc
ACGT = set("ACGT")
MAX_KMERS = ER.MAX_KMERS  # 65 535: the last checkpoint the list form serves


def bases(kmers):
    """the prefix length that holds `kmers` k-mers (0: one base short of the first)"""
    return kmers + K - 1


# ------------------------------------------------------------------------------------------------ 1. checkpoint seams
def seam_checkpoints(lines):
    """bases: one below k and exactly k; one k-mer apart across the seam of a batch of slots (32 slots of four lines, else 64) and of a
    tile (64 k-mers); inside the second and third tile; and two beyond every read of SR.Planted (at most 200 k-mers)"""
    batch = 32 if lines == 4 else 64
    kmers = sorted({0, 1, batch - 1, batch, batch + 1, 63, 64, 65, 100, 127, 128, 129, 150})
    return tuple(bases(n) for n in kmers) + (bases(200) + 94, 1000)


ONE_CHECKPOINT = (bases(100),)
SIXTY_FOUR = tuple(K - 1 + 3 * i for i in range(64))  # 6, 9, ... 195 bases: every lane holds a checkpoint, ranges of three k-mers


def seam_reads(f):
    """SR.Planted's reads: a read of 70 to 200 k-mers per bin of SR.scan_bins() and its reverse complement, and strands of 1 to 71"""
    return f.reads() + f.tail_reads()


# ------------------------------------------------------------------------------------------------ 2. strands and bins
HEAD, TAIL_FROM, MOVE_KMERS = 60, 20, 150
MOVE_CHECKPOINTS = tuple(bases(n) for n in (10, 40, 60, 79, 80, 81, 100, 150))


def strand_pairs(n_bins):
    """(A, B): both halves of the first and of the last counter dword, and the first and last bin of lane 63's first piece; at an odd
    bin count the last dword's high half is a pad counter, and the pair is the last bin with bin 8 (lane 1's first)"""
    last = (n_bins - 2, n_bins - 1) if n_bins % 2 == 0 else (n_bins - 1, 8)
    return [(0, 1), (1, 0), (504, 511), (511, 504), last, last[::-1]]


class Moves:
    """SR's random fill, and per pair (A, B) of strand_pairs() two reads of MOVE_KMERS k-mers:
      whole  its first HEAD k-mers planted forward in A and its whole reverse complement in B: strand 1 counts every k-mer in B, strand 0
             the head in A -- a tie at best up to HEAD k-mers, from there on strand 1 and bin B hold the maximum alone;
      tail   its first HEAD k-mers planted forward in A, and the reverse complement of its k-mers from TAIL_FROM on in B: strand 0 and
             bin A hold the maximum over the head, strand 1 and bin B at the read's end.
    The pairs share bins, so a planted bin holds several reads and counts some k-mers it was not given; where the maximum stands at
    which checkpoint is asserted on the oracle (tests/test_prefix_lists_cpu.py).  A and B are bins of SR.scan_bins()."""

    def __init__(self, n_bins, lines, words):
        self.n_bins, self.lines = n_bins, lines
        SR.random_fill(words, n_bins, SR.N_BLOCKS, ER.load_of(n_bins, lines), seed=n_bins + lines)
        self.o = SR.wrap(n_bins, words)
        rng = np.random.default_rng(n_bins * 32 + lines)
        self.pairs = strand_pairs(n_bins)
        self.whole, self.tail = [], []
        used = set()
        for a, b in self.pairs:
            x, y = (SR.distinct_read(rng, bases(MOVE_KMERS), used) for _ in range(2))
            self.o.insert(po.encode(x[:bases(HEAD)]), a)
            self.o.insert(po.encode(rc(x)), b)
            self.o.insert(po.encode(y[:bases(HEAD)]), a)
            self.o.insert(po.encode(rc(y[TAIL_FROM:])), b)
            self.whole.append(x)
            self.tail.append(y)

    def reads(self):
        return self.whole + self.tail


def strand_maxima(o, read, checkpoints):
    """-> per checkpoint (forward maximum, its lowest bin, reverse maximum, its lowest bin) of the prefix"""
    out = []
    for c in checkpoints:
        e = po.encode(read[:c])
        fwd, rev = o.count(e), o.count(po.revcomp(e))
        out.append((int(fwd.max()), int(fwd.argmax()), int(rev.max()), int(rev.argmax())))
    return out


# ------------------------------------------------------------------------------------------------ 3. the counter edge
def edge_read():
    """65 535 k-mers, the longest last checkpoint the list form serves"""
    return PE.sequence()[:bases(MAX_KMERS)]


EDGE_CHECKPOINTS = (bases(MAX_KMERS - 1), bases(MAX_KMERS))  # a bin set in every block stands at 0xFFFE, then at 0xFFFF
OVER_CHECKPOINTS = (bases(MAX_KMERS), bases(MAX_KMERS + 1))  # a last checkpoint of 65 536 k-mers: the plain form


# ------------------------------------------------------------------------------------------------ 4. who takes which item
C_LAST = 200
MIXED_CHECKPOINTS = (K - 1, K, bases(64), bases(65), 134, C_LAST)
ODD_START = 3
WIDE_BOUND, UNDERSTATED = 400, 150  # the descriptor's max_len: at or beyond the last checkpoint, and below it
UNDER_LEN = 180
KINDS = ("free_short", "free_long", "n_before_last", "n_at_last", "n_first", "short", "empty", "beyond", "under")


def takes(read, c_last, chunk_start=0, max_len=None, chunk_length=0):
    """the take rule of rb_engine_set_prefix_lists for one item: its status so far is RB_OK (the chunk begins within the read), the
    w = min(bases the descriptor selects, c_last) bases the pass looks at lie within the call's bound min(max_len, c_last), and all of
    them are ACGT; any length"""
    if chunk_start > len(read):
        return False
    body = read[chunk_start:chunk_start + chunk_length] if chunk_length else read[chunk_start:]
    w = min(len(body), c_last)
    if max_len is not None and w > min(max_len, c_last):
        return False
    return set(body[:w]) <= ACGT


def taken_counts(reads, c_last, **kw):
    """-> (items the list form takes, items it leaves)"""
    t = [takes(r, c_last, **kw) for r in reads]
    return sum(t), len(t) - sum(t)


def mixed_items(chunk_start=0, seed=9):
    """-> (reads, kinds): one item of every kind of KINDS between N-free ones, the positions counted from chunk_start; "beyond" is a read
    that ends before chunk_start (with chunk_start 0 there is none, and the item is one more empty read); "under" is N-free and
    UNDER_LEN bases long: within the last checkpoint, beyond an understated max_len"""
    rng = np.random.default_rng(seed + chunk_start)
    pad = H.random_dna(rng, chunk_start)

    def with_n(s, at):
        return s[:at] + "N" + s[at + 1:]

    body = {"free_short": H.random_dna(rng, 120), "free_long": H.random_dna(rng, 330),
            "n_before_last": with_n(H.random_dna(rng, 300), C_LAST - 1), "n_at_last": with_n(H.random_dna(rng, 300), C_LAST),
            "n_first": with_n(H.random_dna(rng, 90), 0), "short": H.random_dna(rng, K - 1), "empty": "", "under": H.random_dna(rng, UNDER_LEN)}
    reads, kinds = [], []
    for kind in KINDS:
        reads.append(pad[:max(0, chunk_start - 1)] if kind == "beyond" else pad + body[kind])
        kinds.append(kind)
        reads.append(pad + H.random_dna(rng, int(rng.integers(K, 140))))  # interleaved: an N-free item the kernel takes under any bound
        kinds.append("free_short")
    return reads, kinds


def want_taken(kind, chunk_start, max_len):
    """what the issue's rule says of each kind, spelled out"""
    if kind in ("n_before_last", "n_first"):
        return False
    if kind == "beyond":
        return chunk_start == 0  # (an empty read then)
    if kind in ("free_long", "n_at_last"):
        return max_len >= C_LAST  # w = C_LAST
    if kind == "under":
        return max_len >= UNDER_LEN
    return True
