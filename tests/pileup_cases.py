"""Seeded pileup read sets that sit on the edges of csrc/pileup_kernels.hip: the feature space up to F = 10 240, count
windows that need rounds, reads and ops on window and piece boundaries, the 16-bit / 32-bit counter switch, and the
layout scan's tiles.  Builders only: no GPU, no library call.  tests/test_pileup_edges_cpu.py asserts on the restatement
(tests/pileup_ref.py) alone that each set is what it claims to be; tests/test_pileup_edges_gpu.py compares the kernels.

The kernel's sizing is restated here as plain Python (PC_LDS_WORDS, PC_SUB, PT_TILE, window, cap16, cap32): a change of
those constants has to be repeated here, and the CPU test then says which claim no longer holds."""
import functools
from types import SimpleNamespace

import numpy as np

import pileup_ref as PR
from genomicsbench_amd.pileup import PileupReads, n_features

M, I, D, N, S, H, Pd, EQ, X = range(9)
PC_LDS_WORDS = 16384                     # 64 KiB of LDS counters per workgroup
PC_SUB = 32                              # positions per task ("piece")
PT_TILE = 8192                           # positions per scan tile
WIDE_FROM = 65535                        # candidates from which a window counts in 32 bits
BASES = np.array([1, 2, 4, 8], dtype=np.uint8)                                    # A C G T
IUPAC = np.array([0, 3, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15], dtype=np.uint8)      # = M R S V W Y H K D B N: count nothing
A_, C_ = 1, 2


def window(F):
    """positions per count window"""
    return max(PC_SUB, min(512, (2 * PC_LDS_WORDS // F) // 2 // PC_SUB * PC_SUB))


def cap16(F):
    """columns per round with two 16-bit counters a dword"""
    return 2 * PC_LDS_WORDS // F


def cap32(F):
    """columns per round with one counter a dword"""
    return PC_LDS_WORDS // F


# ------------------------------------------------------------------------------------------------- what the kernel sees
def read_ends(reads):
    """end (exclusive) of every read on the reference, from its CIGAR"""
    ops, lens = reads.cigar & 15, (reads.cigar >> 4).astype(np.int64)
    ref = np.where(np.isin(ops, PR.REF_OPS), lens, 0)
    assert (np.diff(reads.cigar_off) > 0).all()
    return reads.pos.astype(np.int64) + np.add.reduceat(ref, reads.cigar_off[:-1])


def candidates(reads, w0, w1):
    """the read range [r_lo, r_hi) that the count kernel walks for the window [w0, w1): the reads with pos < w1, from the
    first whose prefix maximum of ends is > w0"""
    pmax = np.maximum.accumulate(read_ends(reads))
    r_hi = int(np.searchsorted(reads.pos, w1, "left"))
    r_lo = int(np.searchsorted(pmax[:r_hi], w0, "right"))
    return r_lo, r_hi


def windows(p0, p1, F):
    W = window(F)
    return [(w0, min(w0 + W, p1)) for w0 in range(p0, p1, W)]


def round_edges(pos_col, start, w0, w1, cap):
    """the columns at which a later round of the window [w0, w1) starts"""
    c_lo, c_hi = int(pos_col[w0 - start]), int(pos_col[w1 - start])
    return list(range(c_lo + cap, c_hi, cap))


def cigar_ops(reads, r):
    """[(k, op, reference position of its start, len)] of read r, every op"""
    pos, cig = reads.read(r)[:2]
    out, rp = [], pos
    for k, (op, ln) in enumerate(cig):
        out.append((k, op, rp, ln))
        if op in PR.REF_OPS:
            rp += ln
    return out, cig


# ------------------------------------------------------------------------------------------------- building reads
def qlen(cigar):
    return sum(ln for op, ln in cigar if op in PR.QUERY_OPS)


def rlen(cigar):
    return sum(ln for op, ln in cigar if op in PR.REF_OPS)


def rec(rng, pos, cigar, rev=0, dtype=0, quals=None, base=None, iupac=0.0):
    """quals: None (1..60), one value, or the values to draw from; base: one nt16 code for every base, or random ACGT"""
    n = qlen(cigar)
    seq = BASES[rng.integers(0, 4, n)] if base is None else np.full(n, base, dtype=np.uint8)
    if iupac:
        odd = rng.random(n) < iupac
        seq[odd] = IUPAC[rng.integers(0, IUPAC.size, int(odd.sum()))]
    if quals is None:
        q = rng.integers(1, 61, n)
    elif np.isscalar(quals):
        q = np.full(n, quals)
    else:
        q = rng.choice(np.asarray(quals), n)
    return dict(pos=int(pos), cigar=[(op, int(ln)) for op, ln in cigar], seq=seq, qual=q.astype(np.uint8), rev=int(rev), dtype=int(dtype))


def build(recs):
    return PileupReads.from_records(sorted(recs, key=lambda r: r["pos"]))          # (stable)


def expand(recs, mult):
    """recs (sorted by pos) with recs[c] repeated mult[c] times, copies next to each other: 65 k dicts would be slow"""
    cls = PileupReads.from_records(recs)
    assert (np.diff(cls.pos) >= 0).all()
    rep = np.asarray(mult, dtype=np.int64)
    off = lambda per: np.concatenate([[0], np.cumsum(np.repeat(per, rep))])  # noqa: E731
    lens = np.diff(cls.seq_off)
    nbytes = (lens + 1) // 2
    tiles = lambda a, o0, o1: np.concatenate([np.tile(a[o0[c]:o1[c]], rep[c]) for c in range(len(recs))])  # noqa: E731
    return PileupReads(np.repeat(cls.pos, rep), off(np.diff(cls.cigar_off)), tiles(cls.cigar, cls.cigar_off[:-1], cls.cigar_off[1:]),
                       off(lens), off(nbytes)[:-1], tiles(cls.seq, cls.seq_boff, cls.seq_boff + nbytes),
                       tiles(cls.qual, cls.seq_off[:-1], cls.seq_off[1:]), np.repeat(cls.rev, rep), np.repeat(cls.dtype, rep))


def reference(case):
    """-> (pos_col, stats, major, minor, counts) of the whole region from the restatement; computed once per case.  A case
    with `mult` is restated from its distinct reads (scaled_reference)."""
    if getattr(case, "_ref", None) is None:
        if case.mult is not None:
            case._ref = scaled_reference(case.recs, case.mult, case.start, case.end, case.nd, case.nh)
        else:
            pc, st = PR.layout(case.reads, case.start, case.end, case.nd)
            case._ref = (pc, st) + PR.counts(case.reads, case.start, case.end, pc, case.nd, case.nh)
        for a in case._ref:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return case._ref


def layout_reference(case):
    """-> (pos_col, stats) alone, for the cases whose counts are not compared"""
    if getattr(case, "_lref", None) is None:
        case._lref = PR.layout(case.reads, case.start, case.end, case.nd)
    return case._lref


def scaled_reference(recs, mult, start, end, nd, nh):
    """The restatement of expand(recs, mult) from one copy of each read.  Every count is a sum over reads of what one read
    adds, and a position has columns where any read spans it, as many as the longest insertion there: so pos_col, n_cols,
    n_positions and max_ins are those of one copy each, and depth, aligned bases and counts are the single reads' values
    times mult.  test_pileup_edges_cpu.py checks this against the restatement of the expanded reads for mult <= 50."""
    cls = PileupReads.from_records(recs)
    pc, st = PR.layout(cls, start, end, nd)
    major, minor, _ = PR.counts(cls, start, end, pc, nd, nh)
    depth = np.zeros(end - start, dtype=np.int64)
    cnt = np.zeros((int(pc[-1]), n_features(nd, nh)), dtype=np.int64)
    aligned = 0
    for c, m in enumerate(mult):
        one = PileupReads.from_records([recs[c]])
        pc1, st1 = PR.layout(one, start, end, nd)
        depth += int(m) * (np.diff(pc1) > 0)
        aligned += int(m) * st1["aligned_bases"]
        cnt += int(m) * PR.counts(one, start, end, pc, nd, nh)[2].astype(np.int64)
    assert cnt.max() < 2 ** 32
    st = dict(st, max_depth=int(depth.max()), aligned_bases=int(aligned))
    return pc, st, major, minor, cnt.astype(np.uint32)


def _case(name, reads, start, end, nd, nh, recs=None, mult=None, **more):
    return SimpleNamespace(name=name, reads=reads, start=start, end=end, nd=nd, nh=nh, F=n_features(nd, nh), recs=recs, mult=mult,
                           _ref=None, **more)


# ------------------------------------------------------------------------------------------------- 1. the feature space
FEATURE_GRID = [(1, 1), (1, 64), (64, 1), (3, 7), (4, 13), (16, 64), (64, 16)]


@functools.lru_cache(maxsize=None)
def feature_grid(nd, nh):
    """72 reads over 200 positions, both strands, dtype r % nd.  Two reads in three draw their qualities from {0, 1, nh - 1,
    nh, nh + 1, 254, 255}, which reach only the strata 0, nh - 2 and nh - 1; the third takes 1, 2, .. nh, 1, .. along its
    bases from an offset of its own, so that every stratum is reached."""
    rng = np.random.default_rng(100 * nd + nh)
    start, n = 3001, 200
    qset = sorted({min(255, max(0, q)) for q in (0, 1, nh - 1, nh, nh + 1, 254, 255)})
    recs = []
    for r in range(72):
        span = int(rng.integers(40, 90))
        pos = start - 15 + int(rng.integers(0, n - 20))
        a = int(rng.integers(3, span - 12))
        cigar = [[(M, span)],
                 [(M, a), (I, int(rng.integers(1, 9))), (M, span - a)],
                 [(M, a), (D, int(rng.integers(1, 6))), (M, span - a)],
                 [(S, 3), (EQ, a), (X, 2), (I, int(rng.integers(1, 9))), (M, span - a), (D, 2), (M, 4), (I, 2)]][r % 4]
        q = rec(rng, pos, cigar, rev=int(rng.integers(0, 2)), dtype=r % nd, quals=qset, iupac=0.05)
        if r % 3 == 2:
            q["qual"] = ((np.arange(q["qual"].size) + 7 * r) % nh + 1).astype(np.uint8)
        recs.append(q)
    return _case("feature_grid[%d-%d]" % (nd, nh), build(recs), start, start + n, nd, nh)


def check_feature_grid(case, ref):
    cnt = ref[4].astype(np.int64).sum(axis=0).reshape(case.nd, case.nh, 10)
    assert (cnt.sum(axis=(1, 2)) > 0).all(), "a dtype without a count"
    assert (cnt.sum(axis=(0, 2)) > 0).all(), "a stratum without a count"
    assert set(case.reads.dtype.tolist()) >= {0, case.nd - 1}
    q = case.reads.qual
    assert (q == 0xFF).any() and ((q >= case.nh) & (q < 0xFF)).any() and (q == 0).any()
    assert np.isin(case.reads.rev, (0, 1)).all() and 0 < case.reads.rev.sum() < case.reads.n_reads
    assert cnt[:, 0, 8].sum() > 0 and cnt[:, 0, 9].sum() > 0 and ref[1]["max_ins"] > 0          # d, D and insertions


# ------------------------------------------------------------------------------------------------- 2. rounds
ROUNDS_F = {10: (1, 1), 100: (2, 5), 520: (4, 13), 10240: (16, 64)}


@functools.lru_cache(maxsize=None)
def rounds(F):
    """Reads that all start at the region's start and span it.  After each of the positions W/2, W - 1 (a window's last), W
    and W + 40 one read has an insertion of cap16 + 5, 2 cap16 + 7, 3 and cap16 bases, a second read one a third as long,
    and a third read a deletion of three positions across it."""
    nd, nh = ROUNDS_F[F]
    rng = np.random.default_rng(F)
    W, cap = window(F), cap16(F)
    start, n = 707, 2 * window(F) + 16
    at = [W // 2, W - 1, W, W + 40]
    ins = [cap + 5, 2 * cap + 7, 3, cap]
    quals = [0, 1, max(1, nh - 1), nh, nh + 1, 255]
    recs = []
    for i, (a, L) in enumerate(zip(at, ins)):
        recs.append(rec(rng, start, [(M, a + 1), (I, L), (M, n - a - 1)], rev=i & 1, dtype=(3 * i) % nd, quals=quals))
        recs.append(rec(rng, start, [(M, a + 1), (I, max(1, L // 3)), (M, n - a - 1)], rev=1 - (i & 1), dtype=(3 * i + 1) % nd, quals=quals))
        recs.append(rec(rng, start, [(M, a - 1), (D, 3), (M, n - a - 2)], rev=(i >> 1) & 1, dtype=(3 * i + 2) % nd if i else nd - 1,
                        quals=quals))
    return _case("rounds[%d]" % F, build(recs), start, start + n, nd, nh, at=[start + a for a in at], ins=ins)


def check_rounds(case, ref):
    pc, F, cap, s = ref[0], case.F, cap16(case.F), case.start
    wins = windows(case.start, case.end, F)
    assert all(r1 - r0 < WIDE_FROM for r0, r1 in (candidates(case.reads, *w) for w in wins))          # 16-bit counters throughout
    ncols = [int(pc[w1 - s] - pc[w0 - s]) for w0, w1 in wins]
    assert max(ncols) > 2 * cap, "no window with three rounds"
    edges = [e for w in wins for e in round_edges(pc, s, *w, cap)]
    inside = [(e, p) for e in edges for p in case.at if pc[p - s] < e < pc[p + 1 - s]]
    assert inside, "no round starts strictly inside one position's columns"
    assert int(np.diff(pc).max()) > cap, "no position with more columns than a round holds"
    # a round that starts among the columns which the longer insertion alone fills (the shorter one ends at L // 3)
    assert any(pc[p - s] + max(1, L // 3) < e <= pc[p - s] + L for e in edges for p, L in zip(case.at, case.ins))
    # a deletion on a position whose column 0 is a round's first column, and deletions on positions with several columns
    starts = {int(pc[w0 - s]) for w0, _ in wins} | set(edges)
    assert any(int(pc[p - s]) in starts for p in case.at)
    if F == 10240:
        assert cap == 3 and cap32(F) == 1 and all(c > cap for c in ncols), "F = 10 240: every window needs rounds"
    assert set(case.reads.dtype.tolist()) >= {0, case.nd - 1} and 0 < case.reads.rev.sum() < case.reads.n_reads


# ------------------------------------------------------------------------------------------------- 3. window and piece edges
EDGES_F = {10: (1, 1), 100: (2, 5)}
PAIRS = {"M>I": ((M,), I), "M>D": ((M,), D), "D>I": ((D,), I), "N": ((N,), I), "=X": ((EQ,), X), "P-then-I": ((M,), Pd)}


def _pair_read(kind, first_start=None, first_last=None):
    """(pos, cigar) of a read with the op pair `kind`, the pair's first op starting at first_start or ending on first_last"""
    body = {"M>I": ([], [(M, 0), (I, 5), (M, 10)]), "M>D": ([], [(M, 0), (D, 3), (M, 10)]), "D>I": ([(M, 5)], [(D, 0), (I, 4), (M, 10)]),
            "N": ([(M, 5)], [(N, 0), (I, 2), (M, 10)]), "=X": ([(M, 5)], [(EQ, 0), (X, 3), (EQ, 6)]),
            "P-then-I": ([], [(M, 0), (Pd, 1), (I, 3), (M, 10)])}[kind]
    lead, (first, *rest) = body
    ln = 4
    cigar = lead + [(first[0], ln)] + rest
    s = first_start if first_start is not None else first_last - ln + 1
    return s - rlen(lead), cigar


@functools.lru_cache(maxsize=None)
def window_edges(F):
    """Read spans and op pairs on w0 and w1 of the second count window and on a piece boundary inside it; one read over
    all of it followed, in sort order, by 300 short reads that end before that window; a stretch without reads and a
    last read, so that sub-ranges can start where there are no columns.  `sub`: the count sub-ranges [p0, p1)."""
    nd, nh = EDGES_F[F]
    rng = np.random.default_rng(7 * F)
    W = window(F)
    start = 4999
    w0, w1, piece = start + W, start + 2 * W, start + W + 2 * PC_SUB
    end = start + 2 * W + 150
    k = [0]

    def add(pos, cigar):
        k[0] += 1
        recs.append(rec(rng, pos, cigar, rev=k[0] & 1, dtype=(k[0] >> 1) % nd, quals=[0, 1, 3, nh, nh + 1, 255], iupac=0.02))

    recs = []
    add(start, [(M, 2 * W + 100)])
    for i in range(300):
        add(start + i * (W - 21) // 300, [(M, 20)])
    for b in (w0, w1, piece):
        for d in (-1, 0, 1):
            add(b + d, [(M, 20)])                       # the span starts at b - 1, b, b + 1
            add(b + d - 20, [(M, 12), (I, 1), (M, 8)])  # ... ends there
    for kind in PAIRS:
        add(*_pair_read(kind, first_last=w1 - 1))
        add(*_pair_read(kind, first_start=w0))
    add(start + 2 * W + 120, [(M, 20)])
    reads = build(recs)
    p_ins, p_gap = w0 + 3, start + 2 * W + 105            # the M>I pair starting at w0 is 4M 5I: columns after w0 + 3
    sub = [(p_ins, p_ins + L) for L in (1, 31, 32, 33, W - 1, W, W + 1)]
    sub += [(p_gap, p_gap + 33), (start, start + 1), (start, start + W + 1), (start + 5, start + 5 + W)]
    sub += [(end - L, end) for L in (1, 33, W + 1)]
    return _case("window_edges[%d]" % F, reads, start, end, nd, nh, w0=w0, w1=w1, piece=piece, sub=sub, p_ins=p_ins, p_gap=p_gap)


def check_window_edges(case, ref):
    pc, rs, s, W = ref[0], case.reads, case.start, window(case.F)
    assert windows(case.start, case.end, case.F)[1] == (case.w0, case.w1) and (case.piece - case.w0) % PC_SUB == 0
    assert case.w0 < case.piece < case.w1
    ends = read_ends(rs)
    for b in (case.w0, case.w1, case.piece):
        for d in (-1, 0, 1):
            assert (rs.pos == b + d).any(), "no read starts at %d" % (b + d)
            assert (ends == b + d).any(), "no read ends at %d" % (b + d)
    assert (ends == case.w0).any() and (rs.pos == case.w1).any()
    # the op pairs: their first op's last position is w1 - 1, and another's first position is w0
    found = set()
    for r in range(rs.n_reads):
        ops, cig = cigar_ops(rs, r)
        for (k, op, rp, ln) in ops[:-1]:
            for kind, (first, second) in PAIRS.items():
                if op in first and cig[k + 1][0] == second and (kind != "P-then-I" or cig[k + 2][0] == I):
                    if rp + ln - 1 == case.w1 - 1:
                        found.add((kind, "last"))
                    if rp == case.w0:
                        found.add((kind, "first"))
    assert found == {(kind, w) for kind in PAIRS for w in ("last", "first")}, found
    # one read over everything, then 300 candidates by pmax that end before the second window
    assert rs.pos[0] == s and ends[0] > case.w1 and (ends[1:301] <= case.w0).all() and (rs.pos[1:301] >= s).all()
    r_lo, r_hi = candidates(rs, case.w0, case.w1)
    assert r_lo == 0 and r_hi > 301 and (ends[r_lo:r_hi] <= case.w0).sum() >= 300
    # the sub-ranges
    assert pc[case.p_ins + 1 - s] - pc[case.p_ins - s] > 1 and pc[case.p_gap + 1 - s] == pc[case.p_gap - s]
    assert {p1 - p0 for p0, p1 in case.sub if p0 == case.p_ins} == {1, 31, 32, 33, W - 1, W, W + 1}
    assert any(p0 == case.p_gap for p0, _ in case.sub) and any(p0 == s for p0, _ in case.sub) and any(p1 == case.end for _, p1 in case.sub)
    assert all(s <= p0 < p1 <= case.end for p0, p1 in case.sub)


# ------------------------------------------------------------------------------------------------- 4. counter width
COUNTER_WIDTH = ["c65534", "c65535", "a65536", "all65536", "idle", "wide_rounds"]


@functools.lru_cache(maxsize=None)
def counter_width(name):
    """One dtype, one quality.  Reads of 8 reference positions at one pos: `m` forward reads of A only, 3 of C only (A and C
    are the cells 4 and 5 of a column: one dword in 16-bit halves) and a reverse read with a deletion.
      c65534      65 534 candidates: the last 16-bit case
      c65535      65 535: the first 32-bit case
      a65536      m = 65 536: the A cell holds 65 536, which in 16-bit halves is 0 and a carry into C
      all65536    65 536 candidates, no more, every one with a forward A in the first column (three are A then C): the
                  first candidate count at which a 16-bit cell can wrap
      idle        one long read, then 65 535 short reads that end before the region, then five reads in it: 32-bit counters
                  while every count is small
      wide_rounds F = 100: a read over the window with an insertion of 10 and 65 535 reads across column cap32: 32-bit
                  counters and two rounds"""
    rng = np.random.default_rng(len(name))
    q = 7
    if name == "idle":
        start, end = 2600, 3200
        recs = [rec(rng, start - 100, [(M, 700)], quals=q), rec(rng, start - 90, [(M, 8)], base=A_, quals=q),
                rec(rng, start - 50, [(M, 8)], rev=1, base=C_, quals=q)]
        mult = [1, 40000, 25535]
        for i in range(5):
            recs.append(rec(rng, start + 100 * i, [(M, 30), (I, 2 + i), (M, 150), (D, 2), (M, 20)], rev=i & 1, quals=q))
            mult.append(1)
        return _case("counter_width[idle]", expand(recs, mult), start, end, 1, 1, recs, mult, ncand=65541, wide=True, max_depth=4)
    if name == "wide_rounds":
        start, end, at = 2600, 2800, 2750
        recs = [rec(rng, start, [(M, 101), (I, 10), (M, 99)], rev=1, quals=q), rec(rng, at, [(M, 8)], base=A_, quals=q),
                rec(rng, at, [(M, 8)], base=C_, quals=q), rec(rng, at, [(M, 3), (D, 2), (M, 3)], rev=1, quals=q)]
        mult = [1, 65535, 3, 1]
        return _case("counter_width[wide_rounds]", expand(recs, mult), start, end, 1, 10, recs, mult, ncand=65540, wide=True, max_depth=65540)
    start, end, at = 2600, 2640, 2611
    if name == "all65536":
        recs = [rec(rng, at, [(M, 8)], base=A_, quals=q), rec(rng, at, [(M, 8)], base=C_, quals=q)]
        recs[1]["seq"][0] = A_
        mult = [65533, 3]
    else:
        m = {"c65534": 65530, "c65535": 65531, "a65536": 65536}[name]
        recs = [rec(rng, at, [(M, 8)], base=A_, quals=q), rec(rng, at, [(M, 8)], base=C_, quals=q),
                rec(rng, at, [(M, 3), (D, 2), (M, 3)], rev=1, quals=q)]
        mult = [m, 3, 1]
    tot = int(sum(mult))
    return _case("counter_width[%s]" % name, expand(recs, mult), start, end, 1, 1, recs, mult, ncand=tot, wide=tot >= WIDE_FROM, max_depth=tot)


def check_counter_width(case, ref):
    pc, st, _, _, cnt = ref
    rs, s, F = case.reads, case.start, case.F
    assert rs.n_reads == sum(case.mult) and (np.diff(rs.pos) >= 0).all()
    n = [r1 - r0 for r0, r1 in (candidates(rs, *w) for w in windows(case.start, case.end, F))]
    assert n[0] == case.ncand and all((x >= WIDE_FROM) == case.wide for x in n)
    assert st["max_depth"] == case.max_depth
    name = case.name[case.name.index("[") + 1:-1]
    if name in ("c65534", "c65535", "a65536"):
        col = cnt[int(pc[2611 - s])]
        assert col[4] == case.mult[0] and col[5] == 3 and cnt[int(pc[2614 - s]), 8] == 1
        assert (col[4] >= 65536) == (name == "a65536")
    elif name == "all65536":
        assert case.ncand == 65536 and list(cnt[int(pc[2611 - s]), 4:6]) == [65536, 0] and list(cnt[int(pc[2612 - s]), 4:6]) == [65533, 3]
    elif name == "idle":
        assert cnt.max() <= 4 and len(n) == 2 and st["max_ins"] == 6
    else:
        W, cap = window(F), cap32(F)
        assert (W, cap) == (160, 163) and int(pc[s + W - s] - pc[0]) > cap
        edge = round_edges(pc, s, s, s + W, cap)[0]
        assert pc[2750 - s] < edge < pc[2757 - s] and cnt[edge, 64] == 65535 and cnt[edge - 1, 64] == 65535     # the reads lie across it (quality 7: stratum 6, A)


# ------------------------------------------------------------------------------------------------- 5. the layout's scan
SCAN_N = [1, PT_TILE - 1, PT_TILE, PT_TILE + 1, 2 * PT_TILE + 1]
PMAX_READS = [1023, 1024, 1025, 2049]
BIG_N = 1025 * PT_TILE + 3


@functools.lru_cache(maxsize=None)
def scan_edges(n, empty_last_tile=False):
    """A few reads on the edges of the scan tiles of a region of n positions: one across every tile boundary (the depth is
    carried by the tile offsets), one ending on every tile's last position with an insertion there, one ending on the
    region's last position with an insertion (pos_col[n], n_cols), one that starts before the region and one that ends
    after it.  empty_last_tile: nothing reaches the last tile."""
    rng = np.random.default_rng(n)
    start, end = 1234, 1234 + n
    recs = [rec(rng, start - 7, [(M, 4), (I, 2), (M, 4)])]                       # ends at start + 1: position `start` only
    if not empty_last_tile:
        recs.append(rec(rng, max(start - 3, end - 30), [(M, end - 1 - max(start - 3, end - 30)), (I, 3), (M, 1), (I, 5)], rev=1))   # ends at `end`
        recs.append(rec(rng, max(start, end - 11), [(M, 40)]))                   # ends after `end`
    for t in range(1, (n + PT_TILE - 1) // PT_TILE):
        b = start + t * PT_TILE
        if empty_last_tile and b + 60 > start + (n - 1) // PT_TILE * PT_TILE:
            continue
        recs.append(rec(rng, b - 50, [(M, 100)], rev=t & 1))                     # across the boundary
        recs.append(rec(rng, b - 20, [(M, 20), (I, 4)]))                         # its last position is the tile's last
        recs.append(rec(rng, b - 20, [(M, 19), (I, 2), (M, 1)]))                 # an insertion before the tile's last position
    name = "scan_edges[%d%s]" % (n, "-empty" if empty_last_tile else "")
    return _case(name, build(recs), start, end, 1, 5)


def check_scan_edges(case, ref):
    pc, st = ref[0], ref[1]
    n, s, rs = case.end - case.start, case.start, case.reads
    ends = read_ends(rs)
    tiles = (n + PT_TILE - 1) // PT_TILE
    assert (rs.pos < s).any()
    cols = np.diff(pc)
    if case.name.endswith("-empty]"):
        assert tiles == 3 and not cols[(tiles - 1) * PT_TILE:].any() and cols[PT_TILE - 1] == 5 and st["n_cols"] == pc[(tiles - 1) * PT_TILE]
        return
    assert (ends > case.end).any() and cols[n - 1] == 6 and st["n_cols"] == pc[n] and st["max_ins"] == 5
    for t in range(1, tiles):
        b = t * PT_TILE
        assert ((rs.pos < s + b) & (ends > s + b)).any() and cols[b - 1] == 5 and (n == b + 1 or cols[b] == 1)


@functools.lru_cache(maxsize=None)
def pmax_reads(n_reads):
    """The longest read first, over the whole region, then short reads two positions apart, with two longer reads at the
    indices 700 and 701 (with 1025 or 2049 reads a lane of the prefix-maximum kernel takes 2 or 3 reads: 700 = 3 * 233 + 1
    is the middle of a chunk of 3, 701 the second of a chunk of 2).  Every later chunk's maximum comes from chunk 0."""
    rng = np.random.default_rng(n_reads)
    start = 96
    end = start + 2 * n_reads + 40
    recs = [rec(rng, start, [(M, end - start)])]
    for i in range(1, n_reads):
        cigar = [(M, 10), (I, 1 + i % 3), (M, 10)] if i % 5 == 0 else [(M, 20)]
        if i in (700, 701):
            cigar = [(M, min(1500, end - start - 2 * i - 10) if i == 700 else min(900, end - start - 2 * i - 20))]
        recs.append(rec(rng, start + 2 * i, cigar, rev=i & 1))
    return _case("pmax_reads[%d]" % n_reads, build(recs), start, end, 1, 1)


def check_pmax_reads(case, ref):
    rs = case.reads
    ends = read_ends(rs)
    per = (rs.n_reads + 1023) // 1024
    assert per == {1023: 1, 1024: 1, 1025: 2, 2049: 3}[rs.n_reads]
    assert ends[0] == ends.max() == case.end and (ends[1:] < ends[0]).all()
    pm = np.maximum.accumulate(ends[1:])
    assert (pm == ends[700]).sum() > 300 and ends[701] < ends[700]          # the second long read leads a long stretch
    wins = windows(case.start, case.end, case.F)
    assert len(wins) >= 4 and all(candidates(rs, *w)[0] == 0 for w in wins)       # every window walks from read 0


@functools.lru_cache(maxsize=None)
def scan_big():
    """1025 * 8192 + 3 positions: 1026 tiles, so each lane of the tile-sum scan takes two of them.  Twenty reads spread over
    the region, one across the boundary of tiles 1023 and 1024 with an insertion on each side, one long read over 20
    tiles, and one in the last tile that ends on the region's last position with an insertion."""
    rng = np.random.default_rng(1025)
    start, n = 1000, BIG_N
    recs = [rec(rng, start + i * (n // 20) + 17, [(M, 50), (I, 3), (M, 50)], rev=i & 1) for i in range(20)]
    b = start + 1024 * PT_TILE
    recs.append(rec(rng, b - 10, [(M, 10), (I, 2), (M, 1), (I, 4), (M, 9)]))
    recs.append(rec(rng, start + 300 * PT_TILE - 5, [(M, 20 * PT_TILE)]))
    recs.append(rec(rng, start + n - 40, [(M, 40), (I, 6)]))
    return _case("scan_big", build(recs), start, start + n, 1, 5)


def check_scan_big(case, ref):
    pc, st = ref[0], ref[1]
    n = case.end - case.start
    cols = np.diff(pc)
    tiles = (n + PT_TILE - 1) // PT_TILE
    assert tiles == 1026 and (tiles + 1023) // 1024 == 2
    assert cols[n - 1] == 7 and cols[1024 * PT_TILE - 1] == 3 and cols[1024 * PT_TILE] == 5 and st["max_depth"] == 2
    per_tile = np.add.reduceat(cols, np.arange(0, n, PT_TILE))
    assert (per_tile[300:320] >= PT_TILE - 5).all() and per_tile[1025] > 0 and (per_tile == 0).sum() > 900
