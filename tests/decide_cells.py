"""The decision table of check_unblock / classify_reads / Read::classify(std::vector<TIbf>&) (src/main/adaptive_sampling.hpp:35-113,
src/main/classify.hpp:58-111, src/IBF/IBFClassify.cpp:181-365) enumerated cell by cell, and reads designed to land in every cell.

A CELL names the branch a read takes through that logic.  It is computed from the ORACLE's raw maximum per filter, the read length,
each filter's k, the oracle's thresholds at r and at r - 0.02, the mode and (nd, nt) -- never from the code under test:

    (mode, nd>0, nt>0, D1>0, T1>0, D2>0, T2>0, short_d, short_t, tie_d, tie_t, skipped, thr0, wrapped)

D1 / T1: the deplete / target group's max_matches at r; D2 / T2: at r - 0.02; short_g: the read is shorter than the k of the group's
FIRST filter; tie_g: the group's maximum at r is held by two filters (the argmax is strictly-greater: the first must win); skipped: a
filter is passed over because its own k > len while its group's first filter is not; thr0: some filter's threshold at r is 0 (every
read a hit in CLASSIFY_ANY, none in the argmax modes, whose max_matches is then 0); wrapped: some filter's threshold at r is a
negative int16 received as uint16 (65 529 for the 35-mer of the reference's KAT), which no count reaches.

REQUIRED / IMPOSSIBLE.  The full cross product has 3 * 2^13 cells.  Which of them the reference's logic can reach is decided by
`plan()`: an exhaustive enumeration of the MODEL -- every filter set of FILTER_SETS, every error rate of RATES, every length of
LENGTHS, every way the members of the two groups can share a count (SCENARIOS: no member, all members tied, the first alone, the last
alone, at the larger or the smaller of two count levels) and every pair of count levels taken from {0, t - 1, t, all k-mers} over the
oracle's own thresholds t -- pushed through `cell()`.  What the enumeration reaches is REQUIRED; the rest of the cross product is
IMPOSSIBLE, each with the first reason of `why_impossible` that applies.  Two count levels are enough: a cell depends on each group's
maximum at the two thresholds and on whether that maximum is held twice, never on a third distinct count.

The READ DESIGNER turns the enumeration's witnesses into reads.  Every filter of a set is built (add_sequence, one 1 200-base chunk
per bin) from the same list of chunks; chunk c belongs to scenario c, and a filter holds it whole ('F'), holds its left half only
('L', the right half replaced by bases of its own) or not at all ('-').  A window of the chunk with `wb` bases left of the middle and
`wa` in all then counts wa - k + 1 in an 'F' filter, wb - k + 1 in an 'L' filter and nothing elsewhere; the rest of the read is random.
A false positive of the Bloom filter can move a read by one count: the tests compute every cell from the oracle's raw maxima of the
finished read, and assert the reach (>= 3 reads per REQUIRED cell) rather than trusting the design.

Test infrastructure: uses the oracle, never imports the product library."""
import functools
import itertools

import numpy as np

from oracle import pyoracle as po

MODE_CHECK_UNBLOCK, MODE_CLASSIFY_CHUNK, MODE_CLASSIFY_ANY = 0, 1, 2  # enum rb_mode, include/readbouncer_amd.h
MODES = (MODE_CHECK_UNBLOCK, MODE_CLASSIFY_CHUNK, MODE_CLASSIFY_ANY)
RATES = (0.05, 0.1, 0.15)
HALF = 600            # half a chunk: the longest read
FRAG = 2 * HALF       # fragment length of add_sequence = one chunk per bin
# k - 1, k, k + 1 for both k; the 35-mer; the zero-threshold lengths of k = 13, r = 0.1 (123-130) and their neighbours; lengths whose
# threshold at r - 0.02 is BELOW the one at r (the int16 wrap: 89-92 at k = 13, r = 0.1); ordinary lengths up to the longest read
LENGTHS = (0, 5, 12, 13, 14, 15, 16, 17, 30, 35, 52, 60, 90, 100, 122, 123, 126, 130, 131, 150, 186, 200, 250, 270, 300, 420, 500, 600)
FIELDS = ("mode", "nd>0", "nt>0", "D1>0", "T1>0", "D2>0", "T2>0", "short_d", "short_t", "tie_d", "tie_t", "skipped", "thr0", "wrapped")
MIN_READS_PER_CELL = 3
WITNESSES_PER_SET = 8  # reads designed per (cell, filter set): a cell most sets reach gets a dozen, one only a single set reaches gets few

# name -> (k of the deplete filters, k of the target filters, (n_bins, n_blocks) per filter).  Sparse filters (a bin's 1 200 k-mers set
# 1-5 % of its bits) so that the designed counts hold; 64 - 600 bins: one, two, five and ten words per block.
FILTER_SETS = {
    "d1": ((13,), (), ((64, 262147),)),
    "t1": ((), (13,), ((100, 131101),)),
    "d1t1": ((13,), (13,), ((300, 131101), (64, 262147))),
    "d2t2": ((13, 13), (13, 13), ((64, 262147), (100, 131101), (64, 131101), (64, 131101))),  # scenario 'FF' of a group: a tie
    "d3t1": ((13, 13, 13), (13,), ((64, 131101), (64, 131101), (600, 65537), (100, 131101))),  # scenario '--F': the last one is best
    "d13t15": ((13,), (15,), ((64, 262147), (100, 131101))),      # lengths 13 and 14 are short for the target alone
    "d15t13": ((15,), (13,), ((64, 262147), (100, 131101))),      # ... and for the deplete group alone: the FIRST filter's k is the larger
    "d13d15t13": ((13, 15), (13,), ((64, 262147), (100, 131101), (64, 131101))),  # mixed k inside a group: the second is skipped by its own k
    "d13t15t13": ((13,), (15, 13), ((64, 262147), (100, 131101), (64, 131101))),  # a short read for the target group whose second filter counts
}


def set_ks(name):
    kd, kt, _ = FILTER_SETS[name]
    return tuple(kd) + tuple(kt), len(kd), len(kt)


@functools.lru_cache(maxsize=None)
def threshold(length, k, r):
    return int(po.threshold(int(length), int(k), float(r)))


def thresholds(length, ks, r):
    """the oracle's uint16 thresholds of every filter at r and at r - 0.02 (adaptive_sampling.hpp:55: conf.error_rate -= 0.02)"""
    return tuple(threshold(length, k, r) for k in ks), tuple(threshold(length, k, r - 0.02) for k in ks)


def cell(raw, length, ks, t1, t2, mode, nd, nt):
    """raw[f]: the oracle's raw maximum of filter f (deplete filters first) -> the cell's name (FIELDS)"""
    nf = nd + nt
    assert len(raw) == len(ks) == len(t1) == len(t2) == nf
    # Read::classify(filt1, filt2) skips a filter whose k > len (IBFClassify.cpp:318, 340); max_matches is 0 below the threshold
    c1 = [int(raw[f]) if length >= ks[f] and int(raw[f]) >= t1[f] else 0 for f in range(nf)]
    c2 = [int(raw[f]) if length >= ks[f] and int(raw[f]) >= t2[f] else 0 for f in range(nf)]
    D1, T1 = max(c1[:nd], default=0), max(c1[nd:], default=0)
    D2, T2 = max(c2[:nd], default=0), max(c2[nd:], default=0)
    short_d = nd > 0 and length < ks[0]
    short_t = nt > 0 and length < ks[nd]
    tie_d = D1 > 0 and c1[:nd].count(D1) > 1
    tie_t = T1 > 0 and c1[nd:].count(T1) > 1
    skipped = (nd > 0 and not short_d and any(k > length for k in ks[:nd])) or (nt > 0 and not short_t and any(k > length for k in ks[nd:]))
    thr0 = any(t == 0 for t in t1)
    wrapped = any(t >= 32768 for t in t1)
    return (mode, nd > 0, nt > 0, D1 > 0, T1 > 0, D2 > 0, T2 > 0, short_d, short_t, tie_d, tie_t, skipped, thr0, wrapped)


def cells_of_batch(raw, lens, ks, r, mode, nd, nt):
    """raw: [n, nf] raw maxima of the oracle -> the cell of every read"""
    out = []
    for i, L in enumerate(lens):
        t1, t2 = thresholds(int(L), ks, r)
        out.append(cell(raw[i], int(L), ks, t1, t2, mode, nd, nt))
    return out


def describe(c):
    return "mode %d: " % c[0] + " ".join(n for n, v in zip(FIELDS[1:], c[1:]) if v)


# ---------------------------------------------------------------------------------------------------------------------------------
# the model

def _group_patterns(n):
    if n == 0:
        return [()]
    pats = [("-",) * n]
    for lv in "FL":
        pats.append((lv,) * n)  # every member holds the chunk: equal counts (equal k), a tie
        if n > 1:
            pats.append((lv,) + ("-",) * (n - 1))  # the first alone
            pats.append(("-",) * (n - 1) + (lv,))  # the last alone: the best filter is the last one
    return pats


@functools.lru_cache(maxsize=None)
def scenarios(nd, nt):
    """one tuple of 'F' / 'L' / '-' per filter; scenario c is chunk c of the set's references.  A scenario without an 'F' is one with
    the 'L's turned into 'F's at another window length, so it is left out."""
    return tuple(pd + pt for pd in _group_patterns(nd) for pt in _group_patterns(nt) if "F" in pd + pt)


def _model_raw(sc, ks, wa, wb):
    return [max(0, (wa if lv == "F" else wb if lv == "L" else 0) - k + 1) for lv, k in zip(sc, ks)]


def _window_candidates(length, ks, t1, t2):
    """window lengths that put a filter's count at 0, t - 1, t (for both thresholds of every filter) and at all k-mers"""
    w = {0, length}
    for k, a, b in zip(ks, t1, t2):
        for t in (a, b):
            if 0 < t < 32768:
                w.update((t - 1 + k - 1, t + k - 1))
        w.add(k)  # one k-mer: the smallest count a zero threshold lets through
    return sorted(x for x in w if 0 <= x <= length)


@functools.lru_cache(maxsize=None)
def plan():
    """-> (reached, witnesses): reached = the set of cells WITHOUT the mode that the model reaches; witnesses[set name] = the read
    specifications (length, scenario index or -1 for a random read, wa, wb, rate aimed at) that the designer builds"""
    reached = set()
    seen = {}  # cell -> {set name: witnesses so far}
    witnesses = {name: [] for name in FILTER_SETS}
    for name in FILTER_SETS:
        ks, nd, nt = set_ks(name)
        scs = scenarios(nd, nt)
        for r, L in itertools.product(RATES, LENGTHS):
            t1, t2 = thresholds(L, ks, r)
            cands = _window_candidates(L, ks, t1, t2)
            specs = [(-1, 0, 0)]
            for si, sc in enumerate(scs):
                if "L" in sc:
                    specs += [(si, wa, wb) for wa in cands for wb in cands if 0 < wb <= wa and wb <= HALF and wa - wb <= HALF]
                else:
                    specs += [(si, wa, 0) for wa in cands if wa > 0]
            for si, wa, wb in specs:
                raw = [0] * len(ks) if si < 0 else _model_raw(scs[si], ks, wa, wb)
                c = cell(raw, L, ks, t1, t2, 0, nd, nt)[1:]
                reached.add(c)
                have = seen.setdefault(c, {})
                if have.get(name, 0) < WITNESSES_PER_SET:
                    have[name] = have.get(name, 0) + 1
                    witnesses[name].append((L, si, wa, wb, r))
    return frozenset(reached), {k: tuple(dict.fromkeys(v)) for k, v in witnesses.items()}


def all_cells():
    return [(m,) + bits for m in MODES for bits in itertools.product((False, True), repeat=len(FIELDS) - 1)]


def why_impossible(c):
    """one line on why the reference's logic cannot put a read into cell c (called for cells the enumeration did not reach)"""
    _, nd, nt, D1, T1, D2, T2, short_d, short_t, tie_d, tie_t, skipped, thr0, wrapped = c
    if not nd and not nt:
        return "no filter at all: NullFilterException before any count is looked at, and no engine is made of no filter"
    if not nd and (D1 or D2 or short_d or tie_d):
        return "no deplete filter: its maxima are 0, nothing is short for it and nothing ties in it"
    if not nt and (T1 or T2 or short_t or tie_t):
        return "no target filter: its maxima are 0, nothing is short for it and nothing ties in it"
    if (tie_d and not D1) or (tie_t and not T1):
        return "a tie is a maximum above 0 held twice"
    if thr0 and wrapped and not (nd and nt):
        return "oracle thresholds: a set whose filters share one k has one threshold per length, which is 0 or wrapped, not both"
    return ("oracle thresholds: no filter set of FILTER_SETS, rate of RATES, length up to %d and count of at most len - k + 1 k-mers per "
            "filter puts max_matches at r and at r - 0.02 there (exhaustive enumeration, plan())" % HALF)


@functools.lru_cache(maxsize=None)
def required_and_impossible():
    """-> (REQUIRED: sorted list of cells, IMPOSSIBLE: {cell: reason}); together the full cross product"""
    reached, _ = plan()
    required, impossible = [], {}
    for c in all_cells():
        if c[1:] in reached:
            required.append(c)
        else:
            impossible[c] = why_impossible(c)
    return required, impossible


def __getattr__(name):  # REQUIRED / IMPOSSIBLE as module attributes, computed on first use
    if name == "REQUIRED":
        return required_and_impossible()[0]
    if name == "IMPOSSIBLE":
        return required_and_impossible()[1]
    raise AttributeError(name)


# ---------------------------------------------------------------------------------------------------------------------------------
# references and reads

def _dna(rng, n):
    return "".join(np.array(list("ACGT"))[rng.integers(0, 4, size=n)])


_RC = str.maketrans("ACGT", "TGCA")


@functools.lru_cache(maxsize=None)
def references(name):
    """-> (one reference string per filter of the set, the chunks): bin c of every filter is chunk c as that filter holds it"""
    ks, nd, nt = set_ks(name)
    rng = np.random.default_rng(sorted(FILTER_SETS).index(name) + 1000)
    scs = scenarios(nd, nt)
    chunks = [_dna(rng, FRAG) for _ in scs]
    refs = []
    for f in range(nd + nt):
        parts = []
        for c, sc in enumerate(scs):
            if sc[f] == "F":
                parts.append(chunks[c])
            elif sc[f] == "L":
                other = "ACGT"[("ACGT".index(chunks[c][HALF]) + 1 + int(rng.integers(0, 3))) % 4]  # no k-mer runs on past the middle
                parts.append(chunks[c][:HALF] + other + _dna(rng, HALF - 1))
            else:
                parts.append(_dna(rng, FRAG))
        refs.append("".join(parts))
    return refs, chunks


def geometry(name):
    """-> [(n_bins, n_hash, k, n_bits)] per filter, deplete filters first"""
    ks, _, _ = set_ks(name)
    return [(nb, 3, k, ((nb + 63) // 64) * 64 * blocks) for k, (nb, blocks) in zip(ks, FILTER_SETS[name][2])]


def build_oracle_filters(name):
    """the set's filters through the oracle builder -> (deplete list, target list)"""
    refs, _ = references(name)
    _, nd, _ = set_ks(name)
    out = []
    for (nb, h, k, bits), ref in zip(geometry(name), refs):
        f = po.OracleIBF(nb, h, k, bits)
        f.add_sequence(po.encode(ref), FRAG)
        out.append(f)
    return out[:nd], out[nd:]


def design_read(name, spec, rng):
    """a read of the given length that holds a window of `wa` bases of chunk `si`, `wb` of them left of the chunk's middle; the rest is
    random.  Every other read is handed over as its reverse complement (the counts are those of the better strand)."""
    L, si, wa, wb, _ = spec
    if si < 0 or wa == 0:
        return _dna(rng, L)
    _, chunks = references(name)
    ks, nd, nt = set_ks(name)
    start = HALF - wb if "L" in scenarios(nd, nt)[si] else (FRAG - wa) // 2
    window = chunks[si][start:start + wa]
    assert len(window) == wa <= L
    at = int(rng.integers(0, L - wa + 1))
    read = _dna(rng, at) + window + _dna(rng, L - wa - at)
    return read[::-1].translate(_RC) if rng.integers(0, 2) else read


@functools.lru_cache(maxsize=None)
def designed_reads(name):
    """the read set of one filter set: the designer's witnesses, then the fixed edges (the empty read, k - 1, k, k + 1, the 35-mer, the
    zero-threshold lengths, each as a random read and as a window of the first chunk)"""
    _, wit = plan()
    rng = np.random.default_rng(sorted(FILTER_SETS).index(name) + 5000)
    reads = [design_read(name, s, rng) for s in wit[name]]
    for L in (0, 12, 13, 14, 15, 16, 35, 123, 124, 125, 126, 127, 128, 129, 130):
        reads.append(_dna(rng, L))
        reads.append(design_read(name, (L, 0, L, min(L, HALF) // 2, 0.1), rng))
    return tuple(reads)


def pack(reads):
    lens = np.array([len(r) for r in reads], dtype=np.uint32)
    offs = np.zeros(len(reads), dtype=np.uint64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    buf = np.frombuffer(("".join(reads) or "A").encode(), dtype=np.uint8).copy()
    return buf, offs, lens


# ---------------------------------------------------------------------------------------------------------------------------------
# what the oracle answers

def oracle_raw(filters, buf, offs, lens, n_threads=8):
    return np.stack([po.batch_raw_max(f, buf, offs, lens, n_threads) for f in filters], axis=1)


def oracle_expect(odep, otgt, reads, encoded, buf, offs, lens, r, mode, n_threads=8):
    """-> (decision u8[n], status u8[n], best_target i32[n]) of the oracle: batch_check_unblock, classify_read_chunks with one chunk
    covering the read, classify_any over deplete + target; best_target is Read::classify(TargetFilters) (classify_best), -1 when
    that raises or there is no target filter"""
    n = len(reads)
    best = np.full(n, -1, dtype=np.int32)
    if otgt:
        for i, e in enumerate(encoded):
            st, b = po.classify_best(otgt, e, r)
            best[i] = b if st == po.OK else -1
    if mode == MODE_CHECK_UNBLOCK:
        dec, st = po.batch_check_unblock(odep, otgt, buf, offs, lens, r=r, n_threads=n_threads)
        return dec, st, best
    dec, st = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    for i, rd in enumerate(reads):
        if mode == MODE_CLASSIFY_ANY:
            st[i], found = po.classify_any(list(odep) + list(otgt), encoded[i], r)
            dec[i] = 1 if found and st[i] == po.OK else 0
        else:
            res = po.classify_read_chunks(odep, otgt, rd, len(rd), 1, r)
            st[i] = res["status"]
            dec[i] = 1 if res["classified"] and st[i] == po.OK else 0
    return dec, st, best


def ledger_add(ledger, path, cells):
    d = ledger.setdefault(path, {})
    for c in cells:
        d[c] = d.get(c, 0) + 1


def ledger_missing(ledger, path, required):
    d = ledger.get(path, {})
    return [(c, d.get(c, 0)) for c in required if d.get(c, 0) < MIN_READS_PER_CELL]
