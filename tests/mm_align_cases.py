"""Seeded cases for the base-level alignment stage (tests/mm_align_ref.py is the restatement, tests/mm_align_ref.c its C twin for the
larger jobs).  The generators assert their own coverage, so a case that stops exercising its path fails here and not silently.

A case is a Batch: references, reads, regions with their chained anchors, parameters - and, lazily, what the restatement makes of it."""
import functools
import random

import numpy as np

import mm_align_ref as AR
import mm_cases as K

SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 200, 700)
BANDS = (1, 2, 63, 64, 65, 500)
REG_KEYS = ("id", "parent", "score", "subsc", "cnt", "as", "rid", "rev", "rs", "re", "qs", "qe", "mlen", "blen", "n_sub", "mapq", "hash", "read")
PY_CELLS = 4000                                      # a job the Python restatement takes: at most this many cells


class Batch:
    """One call's input, built a read at a time"""

    def __init__(self, **params):
        self.P = AR.params(**params)
        self.refs, self.reads, self.regs, self.reg_off, self.off, self.cax, self.cay, self.n_chained = [], [], [], [0], [0], [], [], []

    def ref(self, text):
        self.refs.append(bytes(text))
        return len(self.refs) - 1

    def read(self, text, slack=0):
        """a new read; slack: anchor slots of the read that are not chained anchors"""
        self.close()
        self.reads.append(bytes(text))
        self.reg_off.append(self.reg_off[-1])
        self.off.append(self.off[-1])
        self.n_chained.append(0)
        self._slack = slack
        return len(self.reads) - 1

    def region(self, rid, rev, anchors, **over):
        """a region of the last read from its anchors [(x, y, span)]; over: fields to overwrite afterwards (invalid regions)"""
        r = len(self.reads) - 1
        a0 = self.n_chained[r]
        for x, y, sp in anchors:
            self.cax.append((rev << 63 | (rid & 0x7fffffff) << 32 | (x & 0xffffffff)) & (1 << 64) - 1)
            self.cay.append(sp << 32 | (y & 0xffffffff))
        self.n_chained[r] += len(anchors)
        self.off[-1] += len(anchors)
        x0, y0, s0 = anchors[0] if anchors else (0, 0, 0)
        x1, y1, _ = anchors[-1] if anchors else (0, 0, 0)
        qlen = len(self.reads[r])
        q0, q1 = y0 + 1 - s0, y1 + 1
        g = dict(id=self.reg_off[-1] - self.reg_off[-2], parent=self.reg_off[-1] - self.reg_off[-2], score=2 * len(anchors) + 40, subsc=0, cnt=len(anchors),
                 rid=rid, rev=rev, rs=max(x0 + 1 - s0, 0), re=x1 + 1, qs=qlen - q1 if rev else q0, qe=qlen - q0 if rev else q1, mlen=17, blen=19, n_sub=0, mapq=60,
                 hash=0x9e3779b9 ^ len(self.regs), read=r)
        g["as"] = a0
        g.update(over)
        self.regs.append(g)
        self.reg_off[-1] += 1
        return g

    def close(self):
        """pad the last read's anchor slots (cax / cay hold a read's chained anchors at off[r], fewer than its slots)"""
        for _ in range(getattr(self, "_slack", 0)):
            self.cax.append(0)
            self.cay.append(0)
            self.off[-1] += 1
        self._slack = 0

    def arrays(self):
        """-> the arguments of mm_align.align_host / align_cpu after the parameters"""
        import genomicsbench_amd.mm_map as MM
        g = np.zeros(len(self.regs), MM.REG_DTYPE)
        for i, r in enumerate(self.regs):
            for k in REG_KEYS:
                g[k][i] = r[k]
        return (g, np.array(self.reg_off, np.int64), np.array(self.off, np.int64), np.array(self.cax, np.uint64), np.array(self.cay, np.uint64),
                np.array(self.n_chained, np.int32), self.reads, self.refs)

    def expected(self, dp=None, z_bytes=None, stats=None):
        return AR.align_batch(self.P, self.regs, self.reg_off, self.off, self.cax, self.cay, self.n_chained, self.reads, self.refs, z_bytes=z_bytes, stats=stats,
                              dp=dp)


def same(got, want):
    """every record field, every CIGAR word and the counts of a call equal to the restatement's"""
    assert got["counts"] == tuple(want["counts"]), (got["counts"], want["counts"])
    assert len(got["alns"]) == len(want["alns"])
    for k in AR.ALN_FIELDS:
        g, w = got["alns"][k].astype(np.int64).tolist(), [a[k] for a in want["alns"]]
        assert g == w, (k, [(i, x, y) for i, (x, y) in enumerate(zip(g, w)) if x != y][:5])
    assert got["cigar"].tolist() == list(want["cigar"])


def resize(rng, s, n):
    s = bytes(s)
    return s[:n] if len(s) >= n else s + K.rand_seq(rng, n - len(s))


def job_cells(tl, ql, w):
    return sum(sum(1 for t in range(max(0, r - ql + 1), min(tl - 1, r) + 1) if AR.in_band(t, r - t, w)) for r in range(tl + ql - 1)) if tl * ql <= 1 << 16 \
        else (tl + ql) * min(w + 1, tl, ql)


@functools.lru_cache(maxsize=None)
def size_pairs():
    """SIZES squared off to about forty pairs: every size with itself, with its neighbours in the list and with both ends"""
    n = len(SIZES)
    pairs = set()
    for i, a in enumerate(SIZES):
        for j in (i, i - 1, i + 1, 0, n - 1):
            if 0 <= j < n:
                pairs.add((a, SIZES[j]))
    out = sorted(pairs)
    assert 36 <= len(out) <= 48, len(out)
    return out


def single_job_batch(bw, kind, small):
    """One region a job: kind 'fill' (two anchors of span 1, max_ext 0 so nothing else runs), 'right' (one anchor at the start, the
    extension LEFT mode) or 'left' (one anchor at the end: the reversed, RIGHT-mode job; the right extension is one base).
    small: only the jobs the Python restatement takes."""
    rng = random.Random(5000 + 10 * bw + len(kind))
    b = Batch(bw=bw, max_ext=0 if kind == "fill" else 5000)
    for tl, ql in size_pairs():
        w = max(bw, abs(tl - ql) + 1) if kind == "fill" else bw
        if small != (job_cells(tl, ql, w) <= PY_CELLS):
            continue
        t = K.rand_seq(rng, tl)
        q = resize(rng, K.mutate(rng, t, 0.12), ql)
        if kind == "fill":
            rid = b.ref(t + b"A")
            b.read(q + b"A")
            b.region(rid, 0, [(0, 0, 1), (tl, ql, 1)])
        elif kind == "right":
            rid = b.ref(t)
            b.read(q)
            b.region(rid, 0, [(0, 0, 1)])
        else:
            rid = b.ref(t[::-1] + b"C")
            b.read(q[::-1] + b"C")
            b.region(rid, 0, [(tl, ql, 1)])
    b.close()
    return b


# ---- composed pairs: a target and a query written side by side from a recipe, with anchors planted where both agree
def compose(rng, recipe, span=15):
    """recipe: ('=', n) or ('=', n, alphabet) equal bases, ('X', n) mismatches, ('D', text or n) target only, ('I', text or n) query only, ('T', text) /
    ('Q', text) literal on one side, ('B', text) literal on both, ('A',) or ('A', span): an anchor ending at the last base written
    -> (target, query, anchors)"""
    t, q, anchors = bytearray(), bytearray(), []
    other = {65: b"C", 67: b"G", 71: b"T", 84: b"A"}
    for step in recipe:
        k = step[0]
        if k == "=":
            s = K.rand_seq(rng, *step[1:])
            t += s
            q += s
        elif k == "B":
            t += step[1]
            q += step[1]
        elif k == "X":
            s = K.rand_seq(rng, step[1])
            t += s
            q += b"".join(other[c] for c in s)
        elif k in "DT":
            t += K.rand_seq(rng, step[1]) if isinstance(step[1], int) else step[1]
        elif k in "IQ":
            q += K.rand_seq(rng, step[1]) if isinstance(step[1], int) else step[1]
        else:
            anchors.append((len(t) - 1, len(q) - 1, step[1] if len(step) > 1 else span))
    return bytes(t), bytes(q), anchors


def add_composed(b, rng, recipe, rev=0, **over):
    t, q, anchors = compose(rng, recipe)
    rid = b.ref(t)
    b.read(K.revcomp(q) if rev else q)
    return b.region(rid, rev, anchors, **over)


@functools.lru_cache(maxsize=None)
def tie_batch():
    """Repeats with one unit deleted or inserted, inside a fill, a right extension and a left extension: the gap must land
    leftmost on the forward strand, and every case must have more than one co-optimal placement (asserted by re-scoring the
    shifted gap with the restatement).  -> (batch, what the restatement makes of it)"""
    rng = random.Random(808)
    b = Batch()
    want = []
    for unit, copies in ((b"A", 10), (b"AC", 7), (b"T", 4)):
        for op in (2, 1):                                             # a unit deleted from the query (D), inserted into it (I)
            tr, qr = unit * copies, unit * (copies - 1)
            if op == 1:
                tr, qr = qr, tr
            rep = [("T", tr), ("Q", qr)]
            for where in ("fill", "right", "left"):
                if where == "fill":
                    recipe = [("=", 30), ("A",), ("B", b"G"), ("=", 24), ("B", b"G")] + rep + [("B", b"G"), ("=", 40), ("A",), ("=", 5)]
                    at = 30 + 1 + 24 + 1
                elif where == "right":
                    recipe = [("=", 30), ("A",), ("B", b"G"), ("=", 24), ("B", b"G")] + rep + [("B", b"G"), ("=", 40)]
                    at = 30 + 1 + 24 + 1
                else:
                    recipe = [("=", 33), ("B", b"G")] + rep + [("B", b"G"), ("=", 40), ("A",), ("=", 6)]
                    at = 33 + 1
                add_composed(b, rng, recipe)
                want.append((len(b.regs) - 1, op, at, at, len(unit)))
    b.close()
    exp = b.expected()
    for gi, op, ts, qs, ln in want:
        a = exp["alns"][gi]
        words = exp["cigar"][a["cigar_off"]:a["cigar_off"] + a["n_cigar"]]
        gaps = [(w & 15, w >> 4) for w in words if w & 15]
        assert gaps == [(op, ln)], (gi, AR.cigar_text(words))
        t, q = a["rs"], a["qs"]
        for w in words:
            if w & 15:
                assert (t, q) == (ts, qs), "region %d: the gap starts at (%d, %d), leftmost is (%d, %d)" % (gi, t, q, ts, qs)
                break
            t, q = t + (w >> 4), q + (w >> 4)
        # more than one co-optimal placement, by the restatement's own scoring: the same gap a unit further right, and again,
        # consumes the same spans and re-scores to the region's DP score (the gap lies inside one job, so the sum of the jobs'
        # scores is the score of the whole CIGAR)
        g = b.regs[gi]
        T, Q = AR.codes(b.refs[g["rid"]])[a["rs"]:a["re"]], AR.oriented(b.reads[g["read"]], g["rev"])[a["qs"]:a["qe"]]
        runs = [(w & 15, w >> 4) for w in words]
        assert len(runs) == 3 and AR.rescore(b.P, T, Q, runs) == (a["dp_score"], len(T), len(Q))
        placements = 1
        while runs[2][1] > ln:
            runs = [(0, runs[0][1] + ln), runs[1], (0, runs[2][1] - ln)]
            if AR.rescore(b.P, T, Q, runs) != (a["dp_score"], len(T), len(Q)):
                break
            placements += 1
        assert placements > 1, "region %d: one placement only, the tie rules are not exercised" % gi
    return b, exp


@functools.lru_cache(maxsize=None)
def gap_batch():
    """Gaps of 19, 20, 21 and 60 bases in both directions inside a fill: the pieces tie at 20, piece 2 is cheaper from 21"""
    rng = random.Random(909)
    b = Batch()
    want = []
    for ln in (19, 20, 21, 60):
        for k in "DI":
            add_composed(b, rng, [("=", 20), ("A",), ("=", 60), (k, ln), ("=", 60), ("A",), ("=", 10)])
            want.append((k, ln))
    b.close()
    exp = b.expected()
    P = b.P
    assert P["q"] + 20 * P["e"] == P["q2"] + 20 * P["e2"] and P["q"] + 21 * P["e"] > P["q2"] + 21 * P["e2"]
    for (k, ln), a in zip(want, exp["alns"]):
        words = exp["cigar"][a["cigar_off"]:a["cigar_off"] + a["n_cigar"]]
        assert [(w & 15, w >> 4) for w in words if w & 15] == [(2 if k == "D" else 1, ln)], AR.cigar_text(words)
        assert a["dp_score"] == P["a"] * a["mlen"] - AR.gap(P, ln) and a["nm"] == ln
    return b, exp


@functools.lru_cache(maxsize=None)
def ambi_batch():
    """An N in an M pair, in an inserted run and in a deleted run"""
    rng = random.Random(1010)
    b = Batch()
    add_composed(b, rng, [("=", 20), ("A",), ("=", 30), ("T", b"N"), ("Q", b"G"), ("=", 30), ("A",), ("=", 8)])
    add_composed(b, rng, [("=", 20), ("A",), ("=", 30), ("I", b"ACNNGT"), ("=", 30), ("A",), ("=", 8)])
    add_composed(b, rng, [("=", 20), ("A",), ("=", 30), ("D", b"ACGNTTA"), ("=", 30), ("A",), ("=", 8)])
    add_composed(b, rng, [("=", 20), ("A",), ("=", 30), ("B", b"n"), ("=", 30), ("A",), ("=", 8)])
    b.close()
    exp = b.expected()
    a = exp["alns"]
    assert [x["n_ambi"] for x in a] == [1, 2, 1, 1]
    assert (a[0]["mlen"], a[0]["blen"], a[0]["nm"]) == (88, 88, 1) and (a[1]["blen"] - a[1]["mlen"], a[1]["nm"]) == (4, 6)
    assert (a[2]["blen"] - a[2]["mlen"], a[2]["nm"]) == (6, 7) and (a[3]["blen"], a[3]["nm"]) == (88, 1)
    return b, exp


@functools.lru_cache(maxsize=None)
def zdrop_batches():
    """-> [(name, batch, expected)] with the outcomes of the extension rules asserted on the restatement's answer"""
    rng = random.Random(1111)
    out = []
    head = [("=", 20), ("A",), ("=", 150)]

    def one(name, recipe, check, **params):
        b = Batch(**params)
        add_composed(b, rng, recipe)
        b.close()
        st = {}
        exp = b.expected(stats=st, dp=AR.dp_job_c)
        check(exp["alns"][0], st)
        out.append((name, b, exp))
    unrelated = head + [("D", 700), ("I", 700)]
    one("dropped", unrelated, lambda a, st: _assert(a["flags"] & 4 and not a["flags"] & 16 and 165 <= a["re"] <= 200 and 165 <= a["qe"] <= 200))
    one("zdrop_off", unrelated, lambda a, st: _assert(not a["flags"] & 20 and 165 <= a["re"] <= 200), zdrop=-1)   # every diagonal runs, the end is the maximum's
    # 150 A's the query lacks, then bases that are never A: crossing the run costs a mismatch a base on every path but the
    # deletion, whose drop of 24 + l stays under zdrop + l e2 only through the l e2 term
    saved = head + [("T", b"A" * 150), ("=", 300, "CGT")]
    one("saved_by_l", saved, lambda a, st: _assert(not a["flags"] & 4 and st.get("saved_by_l", 0) > 0 and a["re"] == 620), zdrop=100)
    one("same_without_room", saved, lambda a, st: _assert(a["flags"] & 4), zdrop=10)
    one("empty", [("T", b"A" * 40), ("Q", b"C" * 40), ("=", 15), ("A",), ("=", 30)],
        lambda a, st: _assert(st.get("empty_ext", 0) > 0 and a["rs"] == 40 and a["qs"] == 40 and not a["flags"] & 10))
    tail = head + [("X", 3)]
    one("end_bonus_0", tail, lambda a, st: _assert(not a["flags"] & 16 and a["qe"] == 170))
    one("end_bonus_20", tail, lambda a, st: _assert(a["flags"] & 16 and a["qe"] == 173), end_bonus=20)
    return out


def _assert(ok):
    assert ok


@functools.lru_cache(maxsize=None)
def region_batch(min_ksw_len, max_ext):
    """Composed regions: clipped target windows at both contig ends, a reverse-strand region, a read with two regions, spans that
    differ (is_hpc = 1 anchors) with anchors closer than half a span (the clamping rule), and invalid regions next to valid ones."""
    rng = random.Random(1212 + min_ksw_len)
    b = Batch(min_ksw_len=min_ksw_len, max_ext=max_ext)
    body = lambda: [("=", 25), ("A", 21), ("=", 40), ("X", 1), ("=", 50), ("A", 15), ("D", 3), ("=", 90), ("A", 15), ("=", 4), ("A", 31), ("=", 70), ("I", 2),
                    ("=", 45), ("A", 19), ("X", 2), ("=", 130), ("A", 15), ("=", 120), ("A", 15)]
    add_composed(b, rng, [("I", 30)] + body() + [("I", 25)])                                      # the contig starts and ends inside the read
    add_composed(b, rng, [("D", 12), ("I", 30)] + body() + [("D", 9), ("I", 25)])                 # windows clipped by the contig: 12 and 9 bases
    add_composed(b, rng, [("=", 60)] + body() + [("=", 80)], rev=1)
    t, q, anchors = compose(rng, [("=", 30)] + body() + [("=", 20)] + body() + [("=", 10)])       # two regions in a read
    rid = b.ref(t)
    b.read(q)
    half = len(anchors) // 2
    b.region(rid, 0, anchors[:half])
    b.region(rid, 0, anchors[half:])
    for bad in ("rid", "rid_neg", "cnt", "range", "x0", "x_big", "y_big", None):                    # invalid next to valid
        t, q, anchors = compose(rng, [("=", 40)] + body() + [("=", 40)])
        rid = b.ref(t)
        b.read(q, slack=2)
        if bad == "rid":
            b.region(1000, 0, anchors)
        elif bad == "rid_neg":
            b.region(-1, 0, anchors)
        elif bad == "cnt":
            b.region(rid, 0, anchors, cnt=0)
        elif bad == "range":
            b.region(rid, 0, anchors, cnt=len(anchors) + 1)
        elif bad == "x0":
            b.region(rid, 0, [(3, anchors[0][1], 15)] + anchors[1:])
        elif bad == "x_big":
            b.region(rid, 0, anchors[:-1] + [(len(t), anchors[-1][1], 15)])
        elif bad == "y_big":
            b.region(rid, 0, anchors[:-1] + [(anchors[-1][0], len(q), 15)])
        else:
            b.region(rid, 0, anchors)
        b.close()
    st = {}
    exp = b.expected(stats=st, dp=AR.dp_job_c)
    fl = [a["flags"] for a in exp["alns"]]
    assert fl.count(64) == 7 and fl[-1] & 1 and all(f & 1 for f in fl[:5])
    if min_ksw_len == 8:
        assert st.get("clamped", 0) > 0, "no anchor closer than half its span"
    if max_ext:
        assert exp["alns"][0]["rs"] == 0 and exp["alns"][0]["re"] == len(b.refs[0]), "the region does not span the contig"
    assert exp["alns"][1]["rs"] <= 16
    n_fills = st.get("fills", 0)                                       # six valid regions of seven anchors, one of them clamped onto the one before
    assert n_fills == 30 if min_ksw_len == 8 else n_fills < 24, n_fills
    return b, exp


LDS_ROW = 512                                        # csrc/mm_align_kernels.hip keeps a job's DP rows in LDS up to this many ints a row


@functools.lru_cache(maxsize=None)
def wide_batches():
    """Jobs whose rows are wider than LDS_ROW, so the device keeps them in the job's room, with diagonals of hundreds of cells:
    a band of 600 around fills and both extensions of 700 and more bases, and at the default band fills that hold a 600-base
    deletion and a 600-base insertion (w = |tl - ql| + 1).  -> [(batch, expected)], the wide jobs counted and asserted."""
    rng = random.Random(1313)
    wide = Batch(bw=600)
    for tl, ql in ((700, 705), (760, 700)):
        t = K.rand_seq(rng, tl)
        q = resize(rng, K.mutate(rng, t, 0.1), ql)
        rid = wide.ref(b"ACGTACGTACGTACGTA" + t + b"A")                # a fill between two anchors, the extensions a few bases
        wide.read(b"ACGTACGTACGTACGTA" + q + b"A")
        wide.region(rid, 0, [(16, 16, 15), (17 + tl, 17 + ql, 1)])
        rid = wide.ref(t)                                              # a right extension over everything
        wide.read(q)
        wide.region(rid, 0, [(0, 0, 1)])
        rid = wide.ref(t[::-1] + b"C")                                 # a left extension over everything
        wide.read(q[::-1] + b"C")
        wide.region(rid, 0, [(tl, ql, 1)])
    wide.close()
    indel = Batch()
    for k in "DI":
        add_composed(indel, rng, [("=", 20), ("A",), ("=", 330), (k, 600), ("=", 330), ("A",), ("=", 10)])
    indel.close()
    out = []
    for b, least in ((wide, 6), (indel, 1)):
        n = 0
        for g in b.regs:
            r = g["read"]
            xs = [(b.cax[b.off[r] + g["as"] + i] & 0xffffffff, b.cay[b.off[r] + g["as"] + i] & 0xffffffff, b.cay[b.off[r] + g["as"] + i] >> 32 & 0xff)
                  for i in range(g["cnt"])]
            for _, _, _, tl, ql, w in AR.plan(b.P, xs, len(b.refs[g["rid"]]), len(b.reads[r])):
                n += tl > 0 and ql > 0 and AR.ring(w, tl) > LDS_ROW and min(tl, ql, w + 1) > 128
        assert n >= least, "%d jobs with rows outside LDS and diagonals of more than two lane trips" % n
        out.append((b, b.expected(dp=AR.dp_job_c)))
    return out


@functools.lru_cache(maxsize=None)
def seeded_batch(min_ksw_len, max_ext, bw=500):
    """The seeded reads of mm_map_cases.map_case() with the regions its restatement makes"""
    import mm_map_cases as MK
    c = MK.map_case()
    b = Batch(min_ksw_len=min_ksw_len, max_ext=max_ext, bw=bw)
    e = c["exp"]
    b.refs, b.reads = [bytes(r) for r in c["refs"]], [bytes(r) for r in c["reads"]]
    b.regs = [{k: int(e["regs"][k][i]) for k in REG_KEYS} for i in range(len(e["regs"]["id"]))]
    b.reg_off, b.off = [int(v) for v in e["reg_off"]], [int(v) for v in c["batch"]["off"]]
    b.cax, b.cay, b.n_chained = [int(v) for v in e["cax"]], [int(v) for v in e["cay"]], [int(v) for v in e["n_chained"]]
    assert any(g["rev"] for g in b.regs) and any(b.reg_off[r + 1] - b.reg_off[r] >= 2 for r in range(len(b.reads)))
    return b


@functools.lru_cache(maxsize=None)
def paf_case():
    """the composed regions with names and rep_len -> the arguments of mm_align.paf_cigar_* and the restatement's text"""
    import genomicsbench_amd.mm_align as MA
    b, want = region_batch(8, 5000)
    g, ro = b.arrays()[:2]
    alns = np.zeros(len(want["alns"]), MA.ALN_DTYPE)
    for i, a in enumerate(want["alns"]):
        for k in AR.ALN_FIELDS:
            alns[k][i] = a[k]
    qn, tn = ["q%d" % i for i in range(len(b.reads))], ["contig_%d" % i for i in range(len(b.refs))]
    so, to = np.cumsum([0] + [len(r) for r in b.reads]), np.cumsum([0] + [len(r) for r in b.refs])
    rep = np.arange(len(b.reads), dtype=np.int32) % 3 * 17
    text = AR.paf_cigar(b.regs, ro, want["alns"], want["cigar"], qn, [len(r) for r in b.reads], tn, [len(r) for r in b.refs], rep)
    return g, ro, alns, np.array(want["cigar"], np.uint32), qn, so, rep, tn, to, text
