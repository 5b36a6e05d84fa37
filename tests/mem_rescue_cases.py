"""Inputs of the mate-rescue tests (gbx_mem_rescue_*), shared by the CPU and the GPU tests: hand-built SW inputs with the outcome
written out beside each, hand-built calls of the stage, one per rule and branch of DESIGN 3.14, and generators of calls on a
genome of 20 kb with two contigs.

The regions of a read are given as coordinates and scores; steps 3 to 5 of tests/mem_regs_ref.py (primary marking with read_id0 =
2 pair_id0, mapq, report) turn them into what the regs stage would hand over.  A job is dict(params, pair_id0, regs, reg_off,
seeds, l_rep, read_off, read_len, text, qer, L, contig_off, pes); a hand-built job has `expect` as well: per pair (n_sw, n_added,
n_kept) and the rescued regions in output order as (read, rb, re, qb, qe, score, csub)."""
import functools
import json
import os

import numpy as np

import mem_regs_ref as RG
import mem_rescue_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
FAILED = (0, 0, 1, 0., 0.)
FR = (100, 500, 0, 300., 50.)
PES_FR = [FAILED, FR, FAILED, FAILED]
PES_ALL = [FR, FR, FR, FR]
REGS_SHARED = ("a", "b", "o_del", "e_del", "o_ins", "e_ins", "max_chain_gap", "min_seed_len", "T", "mapq_coef_len", "mapq_coef_fac",
               "mask_level", "mask_level_redun")


def genome(n, seed):
    return np.random.default_rng(seed).integers(0, 4, n).astype(np.uint8)


def text_of(g):
    return np.concatenate([g, (3 - g[::-1]).astype(np.uint8)])


def rc(s):
    return R.revcomp(s).astype(np.uint8)


# ---- hand-built SW inputs: name -> (q, t, params, (score, te, qe, score2, te2, qb, tb))
def _s(txt):
    return np.array(["ACGTN".index(c) for c in txt], dtype=np.uint8)


def _other(x):
    """A sequence that differs from x at every place (so it extends no match of x)."""
    return ((np.asarray(x) + 2) % 4).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def sw_cases():
    S = {}
    # one row: the first column with the base wins, the third is an entry of its own outside te +- 1
    S["m1"] = (_s("A"), _s("CGATA"), dict(min_seed_len=1), (1, 2, 0, 1, 4, 0, 2))
    # exact copies at column 5; m = 8 and 16 fill slen * 16 rows exactly, 9 and 17 leave 7 and 15 padded rows
    g = genome(60, 901)
    for m in (8, 9, 16, 17):
        q = g[:m].copy()
        S["m%d" % m] = (q, np.concatenate([_other(q[:5]), q, _other(q[:6])]), dict(min_seed_len=5), (m, 4 + m, m - 1, -1, -1, 0, 5))
    # a = 5: 49 rows are 245 < 250 (16 lanes, slen 4, 15 padded rows), 50 rows are 250 (8 lanes, slen 7, 6 padded rows)
    for m in (49, 50):
        S["width_%d" % (5 * m)] = (g[3:3 + m].copy(), g.copy(), dict(a=5), (5 * m, 2 + m, m - 1, -1, -1, 0, 3))
    # a = 1 at the switch itself: 249 rows are 16 lanes with slen 16, 250 rows are 8 lanes with slen 32.  ACGT ends on rows 3 and
    # 16 in the same column with 4 each.  In 16 x 16 row 16 sits at place 0 * 16 + 1 = 1 and row 3 at 3 * 16 = 48: qe = 16.  The
    # reverse pass on those 17 rows (2 x 16) meets the same tie, TGCA ending on rows 3 (place 17) and 16 (place 8): qe' = 16, so
    # qb = 0.  In 8 x 32 row 3 sits at 3 * 8 = 24 and row 16 at 16 * 8 = 128: qe = 3, qb = 0.  A kernel with the other width at
    # either length answers the other qe
    for m, out in ((249, (4, 7, 16, -1, -1, 0, 4)), (250, (4, 7, 3, -1, -1, 0, 4))):
        q = np.concatenate([_s("ACGT"), _s("G" * 9), _s("ACGT"), _s("T" * (m - 17))])
        S["switch_%d" % m] = (q, _s("CCCCACGT" + "C" * 300), dict(min_seed_len=3), out)
    # 32 rows in 2 x 16: row j sits at (j mod 2) * 16 + j div 2.  ACGT ends on rows 3 and 8 in the same column with 4 each: row 3
    # is first by row, row 8 (place 4) is first in striped memory (row 3: place 17)
    q = np.concatenate([_s("ACGT"), _s("G"), _s("ACGT"), _s("T" * 23)])
    S["striped_tie"] = (q, _s("CCCCACGT" + "C" * 30), dict(min_seed_len=3), (4, 7, 8, -1, -1, 5, 4))
    # the query twice in the target: the first column with 25 wins, the second copy is the sub-hit
    q = genome(25, 902)
    t = np.concatenate([_other(q[:5]), q, _other(q[:10]), q, _other(q[:5])])
    S["two_columns"] = (q, t, {}, (25, 29, 24, 25, 64, 0, 5))
    # 32 rows (no padded ones): behind the hit the column maxima fall, first by the mismatches' 4 (28, 24), then along the
    # deletion that leaves the hit (32 - 6 - k: 23, 22, 21, 20, 19, 18).  The run's entry stays at column 36 (28 < 32), so column
    # 38 (24) does not follow the entry's column and makes a second entry, and so do 40 (22) and 42 (20); all lie inside te +- 32
    q = genome(32, 903)
    t = np.concatenate([_other(q[:5]), q, _other(q[:8])])
    S["run_second_entry"] = (q, t, {}, (32, 36, 31, -1, -1, 0, 5))
    # w = 25: a copy of the first 20 rows ending 25 columns behind te lies inside the window, 26 columns behind it outside
    q = genome(25, 904)
    for name, gap, s2 in (("sub_inside", 5, (-1, -1)), ("sub_outside", 6, (20, 55))):
        t = np.concatenate([_other(q[:5]), q, _other(q[:gap]), q[:20], _other(q[20:25])])
        S[name] = (q, t, {}, (25, 29, 24) + s2 + (0, 5))
    # 20 rows (12 padded): the last 19 rows again, ending on the last row exactly w = 20 columns behind te: its own entry lies
    # inside the window, but the padded rows carry the 19 on, and the entry rule, whose entry stays at the run's first column,
    # makes a new entry every other column: the one at + 2 lies outside.  With one column behind the sub-hit there is none
    q = genome(20, 905)
    for name, tail, s2 in (("pad_reach", 2, (19, 46)), ("pad_cut", 1, (-1, -1))):
        t = np.concatenate([_other(q[:5]), q, _other(q[:1]), q[1:], _other(q[:tail])])
        S[name] = (q, t, {}, (20, 24, 19) + s2 + (0, 5))
    # an N in the mate costs 1 and the match it replaces
    q = genome(25, 906)
    t = np.concatenate([_other(q[:5]), q, _other(q[:5])])
    qn = q.copy()
    qn[12] = 4
    S["n_in_mate"] = (qn, t, {}, (23, 29, 24, -1, -1, 0, 5))
    # 18 matches are below min_seed_len * a: no start; 19 are not
    q = genome(19, 907)
    t = np.concatenate([_other(q[:5]), q, _other(q[:5])])
    S["score_18"] = (q[:18].copy(), np.concatenate([_other(q[:5]), q[:18], _other(q[:6])]), {}, (18, 22, 17, -1, -1, -1, -1))
    S["score_19"] = (q, t, {}, (19, 23, 18, -1, -1, 0, 5))
    # free gap opens, b = 5: x against y is an insertion next to a deletion (15 + 15 - 1 - 1), not a mismatch (30 - 5 - 1)
    q = genome(31, 908)
    t2 = q.copy()
    t2[15] = (t2[15] + 1) % 4
    S["ins_del"] = (q, np.concatenate([_other(q[:4]), t2, _other(q[:4])]), dict(b=5, o_del=0, o_ins=0), (28, 34, 30, -1, -1, 0, 4))
    return S


# ---- calls of the stage
class _G:
    """What steps 3 to 5 of mem_regs_ref read and write of a region."""

    def __init__(self, spec, seed, lq, L, contig_off):
        self.rb, self.qb, self.qe, self.score = spec[:4]
        self.re = self.rb + (spec[4] if len(spec) > 4 else self.qe - self.qb)
        fwd = self.rb if self.rb < L else 2 * L - 1 - self.rb
        self.rid = int(np.searchsorted(contig_off, fwd, side="right") - 1)
        self.truesc, self.w, self.seedlen0, self.seedcov, self.seed, self.lq = self.score, 100, 19, 19, seed, lq
        self.roff = max(self.rb - 40, 0)
        self.sub = self.sub_n = self.mapq = self.flag = 0
        self.secondary = self.sel = -1


class Maker:
    def __init__(self, g, contig_off, pes, pair_id0=0, **params):
        self.g, self.L, self.contig_off = g, len(g), np.array(contig_off, dtype=np.int64)
        self.pes, self.pair_id0, self.params = pes, pair_id0, params
        self.regs, self.reg_off, self.seeds, self.l_rep, self.reads, self.n_sel = [], [0], [], [], [], 0
        self.regs_params = RG.params(**{k: v for k, v in params.items() if k in REGS_SHARED})

    def fwd(self, at, n):
        """A read of n bases forward at `at` and its true region (rb, qb, qe, score)."""
        return self.g[at:at + n].copy(), (at, 0, n, n)

    def rev(self, at, n):
        """The reverse complement of the genome's [at, at + n) and its true region."""
        return rc(self.g[at:at + n]), (2 * self.L - (at + n), 0, n, n)

    def pair(self, seq0, regs0, seq1, regs1, l_rep=(0, 0)):
        for e, (seq, specs) in enumerate(((seq0, regs0), (seq1, regs1))):
            r = len(self.reads)
            qoff = sum(len(x) for x in self.reads)
            a = []
            for s in specs:
                x = _G(s, len(self.seeds), len(seq), self.L, self.contig_off)
                a.append(x)
                self.seeds.append((qoff, x.roff, len(seq), x.re - x.rb + 80, x.qb, x.rb - x.roff, 19, 0))
            a = RG.mark_primary(a, 2 * self.pair_id0 + r, self.regs_params)
            RG.report(a, l_rep[e], self.regs_params)
            for x in a:
                if x.flag & 1:
                    x.sel = self.n_sel
                    self.n_sel += 1
                self.regs.append((x.rb, x.re, x.seed, x.qb, x.qe, r, x.rid, x.score, x.truesc, x.sub, x.sub_n, x.w, x.seedcov, x.seedlen0,
                                  x.secondary, x.mapq, x.flag, x.sel, 0))
            self.reg_off.append(len(self.regs))
            self.l_rep.append(l_rep[e])
            self.reads.append(np.asarray(seq, dtype=np.uint8))

    def job(self, expect=None, rescued=None):
        lens = np.array([len(x) for x in self.reads], dtype=np.int32)
        j = dict(params=self.params, pair_id0=self.pair_id0, regs=np.array(self.regs, dtype=R.REG_DTYPE).reshape(-1),
                 reg_off=np.array(self.reg_off, dtype=np.int64), seeds=np.array(self.seeds, dtype=RG.SEED_DTYPE).reshape(-1),
                 l_rep=np.array(self.l_rep, dtype=np.int32), read_off=(np.cumsum(lens) - lens).astype(np.int64), read_len=lens,
                 text=text_of(self.g), qer=np.concatenate(self.reads), L=self.L, contig_off=self.contig_off, pes=self.pes)
        if expect is not None:
            j["expect"], j["rescued"] = expect, rescued
        return j


G20 = genome(20_000, 7001)
CONTIGS = [0, 9_000, 20_000]
L20 = 20_000


def sw_job(q, t, P):
    """The SW input as a call: the target is the genome, the anchor a made-up region at 0, FF alone with [0, n]: one SW of q
    against the whole target."""
    n = len(t)
    assert len(q) < n                                 # the middle of [0, n + len(q)) lies on the forward strand
    m = Maker(np.asarray(t, dtype=np.uint8), [0, n], [(0, n, 0, n / 2., 1.), FAILED, FAILED, FAILED], **P)
    m.pair(genome(20, 77), [(0, 0, 20, 20)], q, [])
    return m.job()


@functools.lru_cache(maxsize=None)
def hand_built():
    J = {}
    # ---- all four directions from a forward anchor at 3000, then FR seen from a reverse anchor.  Every direction is open, so an
    # anchor runs four SWs; one finds the 50-base mate.  In the last pair both ends pair already as FR: each anchor tries the
    # other three directions and finds nothing
    m = Maker(G20, CONTIGS, PES_ALL)
    a0, r0 = m.fwd(3000, 60)
    m.pair(a0, [r0], *(lambda s: (s[0], []))(m.fwd(3300, 50)))       # FF: the mate forward, 300 on
    m.pair(a0, [r0], *(lambda s: (s[0], []))(m.rev(3250, 50)))       # FR: the mate reversed, its far end 299 on
    m.pair(a0, [r0], *(lambda s: (s[0], []))(m.rev(2651, 50)))       # RF: reversed and behind: 3000 - 2700 = 300
    m.pair(a0, [r0], *(lambda s: (s[0], []))(m.fwd(2700, 50)))       # RR: forward and behind
    a1, r1 = m.rev(5240, 60)                                          # the anchor on the reverse strand, rb = 2L - 5300
    m.pair(a1, [r1], *(lambda s: (s[0], []))(m.fwd(5000, 50)))       # its mate forward at 5000: FR, dist 299; found reversed
    x0, y0 = m.fwd(7000, 60)
    x1, y1 = m.rev(7250, 50)
    m.pair(x0, [y0], x1, [y1])
    two_l = 2 * L20
    J["directions"] = m.job([(4, 1, 1)] * 5 + [(6, 0, 0)],
                            [(1, 3300, 3350, 0, 50, 50, -1), (3, two_l - 3300, two_l - 3250, 0, 50, 50, -1),
                             (5, two_l - 2701, two_l - 2651, 0, 50, 50, -1), (7, 2700, 2750, 0, 50, 50, -1), (9, 5000, 5050, 0, 50, 50, -1)])
    # ---- windows.  RR alone from an anchor at 150: [150 - 500, 150 - 100 + 50) is clamped at 0, the mate at 20 is found.  FF alone
    # from a reverse anchor at 2L - 150: [2L - 50, 2L - 150 + 500 + 40) is clamped at 2L, the 40-base mate on [2L - 40, 2L)
    m = Maker(G20, CONTIGS, [FAILED, FAILED, FAILED, FR])
    a, r = m.fwd(150, 60)
    m.pair(a, [r], m.fwd(20, 50)[0], [])
    J["clamp_0"] = m.job([(1, 1, 1)], [(1, 20, 70, 0, 50, 50, -1)])
    m = Maker(G20, CONTIGS, [FR, FAILED, FAILED, FAILED])
    a, r = m.rev(90, 60)
    m.pair(a, [r], m.rev(0, 40)[0], [])
    J["clamp_2L"] = m.job([(1, 1, 1)], [(1, two_l - 40, two_l, 0, 40, 40, -1)])
    # FR from 8600: [8650, 9100) has its middle in contig 0 and is cut at 9000; the mate on [8850, 8900).  From 8800 the middle
    # of [8850, 9300) lies in contig 1: no SW, the pair is copied through
    m = Maker(G20, CONTIGS, PES_FR)
    a, r = m.fwd(8600, 60)
    m.pair(a, [r], m.rev(8850, 50)[0], [])
    a, r = m.fwd(8800, 60)
    m.pair(a, [r], m.rev(8940, 50)[0], [])
    J["contig_edge"] = m.job([(1, 1, 1), (0, 0, 0)], [(1, two_l - 8900, two_l - 8850, 0, 50, 50, -1)])
    # RR from 68: [0, 68 - 100 + 50) has 18 columns, below min_seed_len: no SW.  From 69 it has 19: one SW that finds nothing
    m = Maker(G20, CONTIGS, [FAILED, FAILED, FAILED, FR])
    for at in (68, 69):
        a, r = m.fwd(at, 60)
        m.pair(a, [r], genome(50, 31), [])
    J["window_18_19"] = m.job([(0, 0, 0), (1, 0, 0)], [])
    # ---- anchors.  Four regions of 60, 55, 50 and 40: 40 < 60 - 17 is no anchor, three SWs; max_matesw = 2 leaves two
    for name, kw, n in (("pen_unpaired", {}, 3), ("max_matesw", dict(max_matesw=2), 2)):
        m = Maker(G20, CONTIGS, PES_FR, **kw)
        a, _ = m.fwd(1000, 60)
        m.pair(a, [(1000, 0, 60, 60), (12000, 0, 60, 55), (14000, 0, 60, 50), (16000, 0, 60, 40)], genome(50, 32), [])
        J[name] = m.job([(n, 0, 0)], [])
    # two anchors five bases apart: the first rescues the mate, which then lies 294 from the second: all four set, no second SW
    m = Maker(G20, CONTIGS, PES_FR)
    a, _ = m.fwd(4000, 60)
    m.pair(a, [(4000, 0, 60, 60), (4005, 0, 60, 58)], m.rev(4250, 50)[0], [])
    J["next_anchor_skips"] = m.job([(1, 1, 1)], [(1, two_l - 4300, two_l - 4250, 0, 50, 50, -1)])
    # the mate has a region of 40 on [s, s + 53) reversed, s = 6450: its far end lies 502 from the anchor at 6000, outside, so FR
    # is tried; the window ends at 6500 and holds the mate on [6450, 6500): the rescued 50 covers the 40 on both axes and the
    # dedup removes the original.  The 40 was an anchor too (fixed before any rescue): from it the first read is found again
    # where its region already is, and the copy goes as identical to its predecessor: two added, one kept
    m = Maker(G20, CONTIGS, PES_FR)
    a, r = m.fwd(6000, 60)
    m.pair(a, [r], m.rev(6450, 50)[0], [(two_l - 6503, 0, 50, 40, 53)])
    J["knocks_out_original"] = m.job([(2, 2, 1)], [(1, two_l - 6500, two_l - 6450, 0, 50, 50, -1)])
    # a pair that needs nothing: under FR alone both ends pair already, every anchor has all four set
    m = Maker(G20, CONTIGS, PES_FR)
    x0, y0 = m.fwd(7000, 60)
    x1, y1 = m.rev(7250, 50)
    m.pair(x0, [y0], x1, [y1])
    J["needs_nothing"] = m.job([(0, 0, 0)], [])
    return J


def generated(n_pairs, seed, pair_id0=0, active=0.33, pes=None, lo=30, hi=251, **params):
    """FR pairs cut from the 20 kb genome, reads of lo .. hi bases with a few substitutions; the first end keeps its true region,
    the mate keeps its own with probability 1 - active and otherwise has none or a decoy elsewhere, and now and then an indel."""
    rng = np.random.default_rng(seed)
    m = Maker(G20, CONTIGS, pes or PES_FR, pair_id0=pair_id0, **params)
    for k in range(n_pairs):
        l0, l1 = int(rng.integers(lo, hi + 1)), int(rng.integers(lo, hi + 1))
        frag = max(l0, l1, int(round(rng.normal(300, 40))))
        at = int(rng.integers(0, L20 - frag))
        s0, r0 = m.fwd(at, l0)
        s1, r1 = m.rev(at + frag - l1, l1)
        for s in (s0, s1):
            for x in rng.integers(0, len(s), int(rng.integers(0, 4))):
                s[x] = (s[x] + 1) % 4
        if rng.random() < 0.2:
            x = int(rng.integers(10, l1 - 10))
            s1 = np.delete(s1, x) if rng.random() < 0.5 else np.insert(s1, x, int(rng.integers(0, 4)))
        if k % 11 == 10:
            s0, r0, s1, r1 = s1, r1, s0, r0
        regs0 = [(r0[0], 0, len(s0), len(s0) - int(rng.integers(0, 12)))]
        regs1 = []
        if rng.random() >= active:
            regs1 = [(r1[0], 0, min(len(s1), r1[2]), min(len(s1), r1[2]) - int(rng.integers(0, 12)))]
        elif rng.random() < 0.4:
            regs1 = [(int(rng.integers(0, 2 * L20 - 300)), 0, len(s1), int(rng.integers(20, 40)))]
        if rng.random() < 0.15:
            regs0.append((int(rng.integers(0, 2 * L20 - 300)), 0, len(s0), regs0[0][3] - int(rng.integers(0, 25))))
        m.pair(s0, regs0, s1, regs1, l_rep=(int(rng.integers(0, 20)) * int(rng.random() < 0.2), 0))
    return m.job()


def many_regions(seed=61):
    """A mate with 70 regions (none pairs with the anchor), to which the rescue adds the true one: lists beyond the wave width."""
    rng = np.random.default_rng(seed)
    m = Maker(G20, CONTIGS, PES_FR, pair_id0=9)
    a, r = m.fwd(10_000, 100)
    s1, _ = m.rev(10_150, 100)
    decoys = [(int(rng.integers(0, 9000)) + 150 * k % 7, int(rng.integers(0, 30)), 100 - int(rng.integers(0, 30)), int(rng.integers(19, 45)))
              for k in range(70)]
    m.pair(a, [r], s1, decoys)
    return m.job()


def wide_window(seed=62):
    """One pair under FR in [100, 4000]: a window of about 4 k columns."""
    m = Maker(G20, CONTIGS, [FAILED, (100, 4000, 0, 2000., 500.), FAILED, FAILED])
    a, r = m.fwd(11_000, 120)
    m.pair(a, [r], m.rev(13_500, 100)[0], [])
    return m.job()


@functools.lru_cache(maxsize=None)
def gpu_inputs():
    """name -> job: every generated input tests/test_mem_rescue_gpu.py uses (the CPU test asserts none holds a boundary input)."""
    J = {"one": generated(1, 21, active=1.), "two": generated(2, 22, active=.5), "many": generated(300, 23, pair_id0=400),
         "many_regions": many_regions(), "wide_window": wide_window()}
    for t in range(4):
        J["thread%d" % t] = generated(40, 50 + t, pair_id0=100 * t)
    return J


def p_of(j):
    return R.params(**j["params"])


def reference(j, **caps):
    if not caps:                                      # computed once per job, shared and left unchanged by its users
        if "_ref" not in j:
            j["_ref"] = reference(j, xreg_cap=None)
        return j["_ref"]
    return R.rescue_all(j["regs"], j["reg_off"], j["seeds"], j["l_rep"], j["read_off"], j["read_len"], j["text"], j["qer"], j["L"],
                        j["contig_off"], j["pes"], p_of(j), j["pair_id0"], **caps)


def same(got, want):
    """Byte-exact on the regions, the offsets, the counts, the seed records, the CIGAR list with its tail and the stats; names
    the first difference."""
    for k in ("n_xregs", "n_xseeds", "n_xsel"):
        assert got[k] == want[k], (k, got[k], want[k])
    assert np.array_equal(got["xreg_off"], want["xreg_off"]), "xreg_off"
    for k in ("stats", "xregs"):
        g, w = got[k], want[k]
        assert g.dtype == w.dtype and len(g) == len(w), (k, len(g), len(w))
        for f in w.dtype.names:
            bad = np.nonzero(g[f] != w[f])[0]
            assert len(bad) == 0, "%s.%s differs at %s: %s != %s" % (k, f, bad[:5], g[f][bad[:5]], w[f][bad[:5]])
        assert g.tobytes() == w.tobytes(), k
    for k in ("xseeds", "xsel_seeds", "xsel_res"):
        assert got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), k


def example():
    with open(os.path.join(HERE, "golden", "mem_rescue_example.json")) as f:
        return json.load(f)
