"""Inputs of the paired-end tests (gbx_mem_pair_*), shared by the CPU and the GPU tests: hand-built calls, one per rule and per
branch of the specification with the outcome written out by hand, and generators of calls whose regions are made
up (no index, no extension), among them pairs built to straddle the wave width.

The regions of a read are given as coordinates and scores; steps 3 to 5 of tests/mem_regs_ref.py (primary marking with
read_id0 = 2 pair_id0, mapq, report) turn them into what the regs stage would hand over: gbx_mem_reg records in its output order
and its CIGAR list.  A job is dict(params, pair_id0, regs, reg_off, sel_seeds, sel_res, seeds, l_rep, L, contig_off, pes_in); a
hand-built job has `expect` as well: pes (four (low, high, failed, avg, std), or None where the caller gave them) and per pair
(score, sub, n_sub, n_cand, z0, z1, q_pe, q_se0, q_se1, paired, proper, dir, dist)."""
import functools
import json
import os

import numpy as np

import mem_pair_ref as R
import mem_regs_ref as RG

HERE = os.path.dirname(os.path.abspath(__file__))
L = 100_000
CONTIGS = [0, 50_000, 100_000]
FAILED = (0, 0, 1, 0., 0.)
PES_FR = [FAILED, (100, 500, 0, 300., 50.), FAILED, FAILED]      # what most pairing cases are given: FR, 300 +- 50
PAIR_FIELDS = ("score", "sub", "n_sub", "n_cand", "z0", "z1", "q_pe", "q_se0", "q_se1", "paired", "proper", "dir", "dist")


def reg(strand, x, score, qb=0, qe=100):
    """A region whose pairing key is x: the forward-strand coordinate of its first base ('f') or, on the reverse strand ('r'),
    of its last one."""
    return (strand, x, score, qb, qe)


class _G:
    """What steps 3 to 5 of mem_regs_ref read and write of a region."""

    def __init__(self, spec, seed, lq, L, contig_off):
        strand, x, self.score, self.qb, self.qe = spec
        self.rb = x if strand == "f" else 2 * L - 1 - x
        self.re = self.rb + (self.qe - self.qb)
        self.rid = int(np.searchsorted(contig_off, x, side="right") - 1)
        self.truesc, self.w, self.seedlen0, self.seedcov, self.seed, self.lq = self.score, 100, 19, 19, seed, lq
        self.roff = self.rb - 40
        self.sub = self.sub_n = self.mapq = self.flag = 0
        self.secondary = self.sel = -1


class Builder:
    def __init__(self, pair_id0=0, pes_in=None, L=L, contig_off=CONTIGS, **params):
        self.params, self.pair_id0, self.pes_in, self.L, self.contig_off = params, pair_id0, pes_in, L, np.array(contig_off, dtype=np.int64)
        self.regs, self.reg_off, self.seeds, self.sel, self.l_rep, self.qoff = [], [0], [], [], [], 0
        shared = ("a", "b", "o_del", "e_del", "o_ins", "e_ins", "min_seed_len", "T", "mapq_coef_len", "mapq_coef_fac", "mask_level")
        self.regs_params = RG.params(**{k: v for k, v in params.items() if k in shared})

    def pair(self, end0, end1, l_rep=(0, 0), lq=100):
        for e, specs in enumerate((end0, end1)):
            r = len(self.l_rep)
            a = []
            for s in specs:
                a.append(_G(s, len(self.seeds), lq, self.L, self.contig_off))
                g = a[-1]
                self.seeds.append((self.qoff, g.roff, lq, g.re - g.rb + 80, g.qb, 40, 19, 0))
            a = RG.mark_primary(a, 2 * self.pair_id0 + r, self.regs_params)
            RG.report(a, l_rep[e], self.regs_params)
            for x in a:
                if x.flag & 1:
                    x.sel = len(self.sel)
                    self.sel.append(x)
                self.regs.append((x.rb, x.re, x.seed, x.qb, x.qe, r, x.rid, x.score, x.truesc, x.sub, x.sub_n, x.w, x.seedcov, x.seedlen0,
                                  x.secondary, x.mapq, x.flag, x.sel, 0))
            self.reg_off.append(len(self.regs))
            self.l_rep.append(l_rep[e])
            self.qoff += lq

    def job(self, expect=None):
        seeds = np.array(self.seeds, dtype=RG.SEED_DTYPE).reshape(-1)
        sel_seeds = np.zeros(len(self.sel), dtype=RG.SEED_DTYPE)
        sel_res = np.zeros((len(self.sel), 8), dtype=np.int32)
        for k, x in enumerate(self.sel):
            sel_seeds[k] = seeds[x.seed]
            sel_res[k] = (x.score, x.truesc, x.qb, x.qe, x.rb - x.roff, x.re - x.roff, x.w, 0)
        j = dict(params=self.params, pair_id0=self.pair_id0, regs=np.array(self.regs, dtype=RG.REG_DTYPE).reshape(-1),
                 reg_off=np.array(self.reg_off, dtype=np.int64), sel_seeds=sel_seeds, sel_res=sel_res, seeds=seeds,
                 l_rep=np.array(self.l_rep, dtype=np.int32), L=self.L, contig_off=self.contig_off, pes_in=self.pes_in)
        if expect is not None:
            j["expect"] = expect
        return j


def fr(b, p, dist, s0=100, s1=100, **kw):
    """A forward read at p and its reverse mate an insert of `dist` away, one region each."""
    b.pair([reg("f", p, s0)], [reg("r", p + dist, s1)], **kw)


def ten_fr(b):
    """Ten FR pairs with the inserts 296 .. 305: p25 / p75 = sorted[2] / sorted[7] = 298 / 303, all ten inside [288, 313], avg
    300.5, S = 82.5, std = sqrt(8.25); [283, 318] lies outside avg -+ 4 std = [289.0, 312.0], so the clamps do not fire."""
    for k in range(10):
        fr(b, 1000 + 700 * k, 296 + k)


TEN = (283, 318, 0, 300.5, 8.25 ** .5)
# a lone pair of two perfect reads under TEN: ns = (dist - 300.5) / 2.87; the inserts 296 .. 305 have |ns| <= 1.57, where
# .721 log(2 erfc(|ns| / sqrt 2)) + .499 lies in (-1, 1): q = 200, or 199 where erfc < .25, that is |ns| > 1.15: the inserts 296,
# 297, 304 and 305; score_un = 183: q_pe = raw(17 or 16) = 102 or 96 -> 60, q_se = 60
OF_TEN = [(199 if k in (0, 1, 8, 9) else 200, 0, 0, 1, 0, 0, 60, 60, 60, 1, 1, 1, 296 + k) for k in range(10)]
# the same pair the unpaired way, 60 each
UNPAIRED = (0, 0, 0, 0, 0, 0, 0, 60, 60, 0)


def one(end0, end1, expect, pes_in=PES_FR, pair_id0=0, l_rep=(0, 0), **params):
    b = Builder(pair_id0=pair_id0, pes_in=pes_in, **params)
    b.pair(end0, end1, l_rep=l_rep)
    return b.job(dict(pes=None, pairs=[expect]))


@functools.lru_cache(maxsize=None)
def hand_built():
    """name -> job.  100-base reads under bwa's scoring: a lone perfect hit has mapq 60; tmp = 7; raw(d) = (int)(6.02 d + .499)."""
    J = {}
    # ---- infer_dir: every direction both ways round, all four given as 300 +- 50 so each pair goes the paired way
    every = [(100, 500, 0, 300., 50.)] * 4
    b = Builder(pes_in=every)
    b.pair([reg("f", 1000, 100)], [reg("f", 1300, 100)])          # FF: p2 = 1300 > 1000: 0
    b.pair([reg("f", 3300, 100)], [reg("f", 3000, 100)])          # both forward, the mate behind: 0 ^ 3 = 3
    b.pair([reg("f", 5000, 100)], [reg("r", 5300, 100)])          # FR: p2 = 5300 > 5000: 1
    b.pair([reg("f", 7300, 100)], [reg("r", 7000, 100)])          # the reverse mate behind: 1 ^ 3 = 2
    b.pair([reg("r", 9300, 100)], [reg("f", 9000, 100)])          # seen from the reverse read (b1 = 2L - 1 - 9300): p2 = 2L - 1 - 9000 > b1: 1
    b.pair([reg("r", 11000, 100)], [reg("r", 11300, 100)])        # both reverse: p2 = 2L - 1 - 11300 < b1: 3
    b.pair([reg("r", 13300, 100)], [reg("r", 13000, 100)])        # both reverse the other way: 0
    ok = (200, 0, 0, 1, 0, 0, 60, 60, 60, 1, 1)                   # ns = 0: qd = 200 + .721 log 2 + .499 = 200.999
    J["infer_dir"] = b.job(dict(pes=None, pairs=[ok + (0, 300), ok + (3, 300), ok + (1, 300), ok + (2, 300), ok + (1, 300), ok + (3, 300),
                                                 ok + (0, 300)]))
    # ---- the estimate
    b = Builder()
    ten_fr(b)
    for k in range(9):                                            # nine FF pairs: below ten, failed, the record 0; they go the
        b.pair([reg("f", 20000 + 700 * k, 100)], [reg("f", 20300 + 700 * k, 100)])      # unpaired way and are not proper
    J["nine_against_ten"] = b.job(dict(pes=[FAILED, TEN, FAILED, FAILED], pairs=OF_TEN + [UNPAIRED + (0, 0, 300)] * 9))
    # 220 FR pairs (the ten inserts 22 times: the same percentiles, avg and std) and ten FF pairs: FF has its ten values but
    # 10 < .05 * 220, so it fails and keeps its numbers: inserts 296 .. 305 again
    b = Builder()
    for t in range(22):
        for k in range(10):
            fr(b, 100 + 200 * (10 * t + k), 296 + k)
    for k in range(10):
        b.pair([reg("f", 60000 + 700 * k, 100)], [reg("f", 60296 + 701 * k, 100)])
    J["five_percent"] = b.job(dict(pes=[TEN[:2] + (1,) + TEN[3:], TEN, FAILED, FAILED],
                                   pairs=[OF_TEN[k % 10] for k in range(220)] + [UNPAIRED + (0, 0, 296 + k) for k in range(10)]))
    # heavy tails inside the first bounds: 250 250 290 300 300 300 300 310 350 350: p25 / p75 = 290 / 310, [250, 350] holds all,
    # avg 300, S = 10200, std = sqrt(1020) = 31.9; 4 std = 127.7 reaches past 290 - 60 and 310 + 60: low = (int)(172.25 + .499),
    # high = (int)(427.75 + .499).  ns of the pairs: 0, +-.31, +-1.57: q = 200, 200, 199
    b = Builder()
    wide = [250, 250, 290, 300, 300, 300, 300, 310, 350, 350]
    for k, d in enumerate(wide):
        fr(b, 1000 + 700 * k, d)
    J["four_std_clamps"] = b.job(dict(pes=[FAILED, (172, 428, 0, 300., 1020. ** .5), FAILED, FAILED],
                                      pairs=[(199 if d in (250, 350) else 200, 0, 0, 1, 0, 0, 60, 60, 60, 1, 1, 1, d) for d in wide]))
    # an eleventh pair at 400 whose first end has a second hit of 90 > .8 * 100 over the same bases (cal_sub), and a twelfth
    # with its ends on two contigs: neither counts, the estimate is TEN.  400 lies outside [283, 318]: no candidate; the
    # unpaired way, not proper.  The first end's top has sub = 90, sub_n = 0: mapq = (int)(6.02 * 10 * .7217 + .499) = 43
    b = Builder()
    ten_fr(b)
    b.pair([reg("f", 30000, 100), reg("f", 40000, 90)], [reg("r", 30400, 100)])
    b.pair([reg("f", 49000, 100)], [reg("r", 50300, 100)])
    J["cal_sub_and_contig"] = b.job(dict(pes=[FAILED, TEN, FAILED, FAILED],
                                         pairs=OF_TEN + [(0, 0, 0, 0, 0, 0, 0, 43, 60, 0, 0, 1, 400), UNPAIRED + (0, 1, 1300)]))
    # ---- pairing, under FR 300 +- 50 in [100, 500]
    # the mate 300 away on the next contig: x differs in the rid, dist is far beyond high: no candidate; not proper (rid)
    J["other_contig"] = one([reg("f", 49900, 100)], [reg("r", 50200, 100)], UNPAIRED + (0, 1, 300))
    # std = 1: ns = 100, erfc(70.7) underflows to 0, the log is -inf: a candidate with q = 0, so score = 0 and the pair goes the
    # unpaired way, where 400 in [100, 500] makes it proper
    J["erfc_underflow"] = one([reg("f", 1000, 100)], [reg("r", 1400, 100)], (0, 0, 0, 1, 0, 0, 0, 60, 60, 0, 1, 1, 400),
                              pes_in=[FAILED, (100, 500, 0, 300., 1.), FAILED, FAILED])
    # two mates of 80 at 250 and 350 (ns = -1 and +1: the same q = 180 + (int).171); the hash of Y ^ (pair_id << 8) orders them,
    # and it does so differently for pair 0 and pair 3 (test_every_branch_has_its_case asserts the q tie).  The second mate is
    # secondary to the first whichever it is (equal scores: the regs stage's hash orders them); sub = 180, n_sub = 1; score_un =
    # 163; q_pe = raw(0) - (int)(4.343 log 2 + .499) = 0 - 3 -> 0.  z1 = 0: sub = 80 >= 80: mapq_se 0, min(q_pe, 40) = 0; z1 = 1:
    # secondary, sub taken over = 80: the same.  Pair 0 takes the mate at 250, pair 3 the one at 350
    for name, pid, dist in (("hash_tie_a", 0, 250), ("hash_tie_b", 3, 350)):
        J[name] = one([reg("f", 1000, 100)], [reg("r", 1250, 80), reg("r", 1350, 80)], (180, 180, 1, 2, 0, 0, 0, 60, 0, 1, 1, 1, dist),
                      pair_id0=pid)
    # four mates: 90 at 300 (q 190), 88 at 250 (q 188), 85 at 350 (q 185), 70 at 330 (ns .6: q 170): sub = 188, n_sub counts 188
    # and 185 (188 - 170 > 7).  score_un = 173, q_pe = raw(190 - 188) = 12, less (int)(4.343 log 3 + .499) = 5: 7.  The first end:
    # 60 stays; the mate (sub 88, sub_n 3 within 7... of 90: 88, 85; 70 is not): mapq_se = (int)(6.02 * 2 * .7217 + .499) = 9,
    # less (int)(4.343 log 3 + .499) = 5: 4, which is below q_pe: min(7, 44) = 7
    J["n_sub"] = one([reg("f", 1000, 100)], [reg("r", 1300, 90), reg("r", 1250, 88), reg("r", 1350, 85), reg("r", 1330, 70)],
                     (190, 188, 2, 4, 0, 0, 7, 60, 7, 1, 1, 1, 300))
    # the mate has two hits on two halves of the read, both reported: multi, the unpaired way although q = 150 > 0; the tops are
    # 300 apart: proper.  With the top 600 away (and the other half 300 away: q = 140) it is not
    half = (150, 0, 0, 1, 0, 0, 0, 60, 60, 0, 1, 1, 300)
    J["is_multi_proper"] = one([reg("f", 1000, 100)], [reg("r", 1300, 50, 0, 50), reg("r", 9000, 40, 50, 100)], half)
    J["is_multi_not_proper"] = one([reg("f", 1000, 100)], [reg("r", 1600, 50, 0, 50), reg("r", 1300, 40, 50, 100)],
                                   (140, 0, 0, 1, 0, 0, 0, 60, 60, 0, 0, 1, 600))
    # the mate's top hit (100) lies elsewhere, a secondary one of 60 pairs: q = 160 <= score_un = 183: paired, z = (0, 0), not
    # proper; q_pe = raw(160 - 183) < 0 -> 0; q_se = mapq_se of the tops: 60, and the mate's (sub 60): (int)(6.02 * 40 * .7217 + .499) = 60
    J["below_score_un"] = one([reg("f", 1000, 100)], [reg("r", 30000, 100), reg("r", 1300, 60)],
                              (160, 0, 0, 1, 0, 0, 0, 60, 60, 1, 0, 1, 29000))
    # the same with 95: q = 195 > 183: z1 = 1, a secondary: secondary = -2, sub = 100 >= 95: mapq_se 0; q_pe = raw(12) = 72 -> 60;
    # q_se1 = min(60, 0 + 40) = 40: the + 40 cap
    J["z_on_secondary"] = one([reg("f", 1000, 100)], [reg("r", 30000, 100), reg("r", 1300, 95)],
                              (195, 0, 0, 1, 0, 1, 60, 60, 40, 1, 1, 1, 300))
    # min_seed_len = 5 and a mate of 8 bases scoring 8: q = 108 > score_un = 91, q_pe = raw(17) -> 60; mapq_se = (int)(6.02 * 3
    # + .499) = 18, min(60, 58) = 58, capped by raw(8) = 48
    J["raw_score_cap"] = one([reg("f", 1000, 100)], [reg("r", 1300, 8, 0, 8)], (108, 0, 0, 1, 0, 0, 60, 60, 48, 1, 1, 1, 300),
                             min_seed_len=5)
    # bwa -P: a pair that would pair does not; the unpaired way is never proper then
    J["no_pairing"] = one([reg("f", 1000, 100)], [reg("r", 1300, 100)], UNPAIRED + (0, 1, 300), no_pairing=1)
    # an end with no region, and one whose only region lies below T
    J["empty_end"] = one([reg("f", 1000, 100)], [], (0, 0, 0, 0, 0, -1, 0, 60, 0, 0, 0, -1, 0))
    # 25 < T: z1 = -1.  The pairing still runs: q = 125 > score_un = 108, both reads report their z: paired and proper; q_pe =
    # raw(17) -> 60; the mate's mapq_se = (int)(6.02 * 6 + .499) = 36 -> min(60, 76) = 60
    J["below_T"] = one([reg("f", 1000, 100)], [reg("r", 1300, 25, 0, 25)], (125, 0, 0, 1, 0, 0, 60, 60, 60, 1, 1, 1, 300))
    # l_rep = 30 and 10 of 100 bases: q_pe = (int)(60 * (1 - .5 * .4f) + .499) = 48; mapq_se = 42 lies below it: min(48, 82) = 48;
    # the mate's 54 lies above it and stays
    J["frac_rep"] = one([reg("f", 1000, 100)], [reg("r", 1300, 100)], (200, 0, 0, 1, 0, 0, 48, 48, 54, 1, 1, 1, 300), l_rep=(30, 10))
    # the caller's estimate against what the call would estimate: the ten pairs under FR in [350, 500]: no candidate, not proper
    b = Builder(pes_in=[FAILED, (350, 500, 0, 400., 20.), FAILED, FAILED])
    ten_fr(b)
    J["pes_in_given"] = b.job(dict(pes=None, pairs=[UNPAIRED + (0, 1, 296 + k) for k in range(10)]))
    return J


def synthetic(n_pairs, seed, pair_id0=0, pes_in=None, L=1_000_000, mean=300., sd=30., few=2, **params):
    """Pairs as a run makes them: a fragment with an insert drawn around `mean`, mostly FR, some RF and FF and `few` RR (below
    ten: that direction fails); each end has its true hit and up to three others, some on the same bases (secondaries), some on
    other bases (a second reported hit), a few ends have none."""
    rng = np.random.default_rng(seed)
    b = Builder(pair_id0=pair_id0, pes_in=pes_in, L=L, contig_off=[0, L // 2, L], **params)
    n_rr = 0
    for _ in range(n_pairs):
        u = rng.random()
        kind = "fr" if u < 0.80 else "rf" if u < 0.88 else "ff" if u < 0.96 else "rr"
        if kind == "rr":
            n_rr += 1
            if n_rr > few:
                kind = "fr"
        p = int(rng.integers(1000, L - 3000))
        d = max(120, int(round(rng.normal(mean, sd))))
        ends = []
        for e in (0, 1):
            if kind == "fr":
                true = ("f", p) if e == 0 else ("r", p + d)
            elif kind == "rf":
                true = ("f", p + d) if e == 0 else ("r", p)
            elif kind == "ff":
                true = ("f", p) if e == 0 else ("f", p + d)
            else:
                true = ("f", p + d) if e == 0 else ("f", p)
            regs = []
            if rng.random() > 0.04:
                regs.append(reg(true[0], true[1], int(rng.integers(60, 101))))
            for _ in range(int(rng.integers(0, 4)) * int(rng.random() < 0.5)):
                where = p + int(rng.integers(-600, 600)) if rng.random() < 0.5 else int(rng.integers(1000, L - 3000))
                qb = int(rng.integers(0, 50)) * int(rng.random() < 0.5)
                qe = 100 - int(rng.integers(0, 40)) * int(rng.random() < 0.5)
                regs.append(reg("f" if rng.random() < 0.5 else "r", where, int(rng.integers(10, qe - qb + 1)), qb, qe))
            ends.append(regs)
        b.pair(ends[0], ends[1], l_rep=(int(rng.integers(0, 30)) * int(rng.random() < 0.2), 0))
    return b.job()


def straddle(seed=5):
    """Pairs of 63, 64, 65 and 200 keys (the register sort, its edge, the bitonic network) under a given FR estimate, and one
    whose reverse mate looks back over 90 forward hits closer than `low` before it meets the ones that pair and the one beyond
    `high` that ends the walk."""
    rng = np.random.default_rng(seed)
    b = Builder(pair_id0=40, pes_in=PES_FR)
    for n0, n1 in ((31, 32), (32, 32), (32, 33), (100, 100)):
        base = int(rng.integers(2000, 30000))
        e0 = [reg("f", base + int(rng.integers(0, 900)), int(rng.integers(30, 100))) for _ in range(n0)]
        e1 = [reg("r", base + int(rng.integers(0, 900)), int(rng.integers(30, 100))) for _ in range(n1)]
        b.pair(e0, e1)
    near = [reg("f", 40000 + k, 40 + k % 7) for k in range(90)]                    # 11 .. 100 before the mate: all but one below low
    good = [reg("f", 39700 + 10 * k, 50 + k) for k in range(5)]                    # 360 .. 400 before it
    far = [reg("f", 39000, 99), reg("f", 38000, 98)]                              # beyond high: the first ends the walk
    b.pair(near + good + far, [reg("r", 40100, 90)])
    return b.job()


def extremes():
    """A handful of pairs at max_ins = 1 (only an insert of 1 counts: adjacent forward hits) and at max_ins = 2^20."""
    b1 = Builder(max_ins=1)
    for k in range(12):
        b1.pair([reg("f", 1000 + 500 * k, 100)], [reg("f", 1001 + 500 * k, 100)])
    fr(b1, 20000, 300)
    b2 = Builder(L=8_000_000, contig_off=[0, 8_000_000], max_ins=1 << 20)
    for k in range(12):
        fr(b2, 1000 + 10 * k, (1 << 20) - 37 * k)
    fr(b2, 5000, (1 << 20) + 1)
    fr(b2, 6000, 300)
    return [b1.job(), b2.job()]


@functools.lru_cache(maxsize=None)
def gpu_inputs():
    """name -> job: every generated input tests/test_mem_pair_gpu.py uses (the CPU test asserts none is a boundary input)."""
    J = {"straddle": straddle(), "one": synthetic(1, 11), "two": synthetic(2, 11), "many": synthetic(300, 11),
         "many_id0": synthetic(300, 12, pair_id0=70000, mean=400., sd=45.), "given": synthetic(40, 13, pes_in=PES_FR)}
    J["max_ins_1"], J["max_ins_2_20"] = extremes()
    for t in range(4):
        J["thread%d" % t] = synthetic(150, 40 + t, pair_id0=1000 * t)
    return J


def p_of(j):
    return R.params(**j["params"])


def reference(j, psel_cap=None):
    if psel_cap is None:                              # computed once per job, shared and left unchanged by its users
        if "_ref" not in j:
            j["_ref"] = R.pair_all(j["regs"], j["reg_off"], j["sel_seeds"], j["sel_res"], j["seeds"], j["l_rep"], j["L"], j["contig_off"],
                                   p_of(j), j["pair_id0"], j["pes_in"])
        return j["_ref"]
    return R.pair_all(j["regs"], j["reg_off"], j["sel_seeds"], j["sel_res"], j["seeds"], j["l_rep"], j["L"], j["contig_off"], p_of(j),
                      j["pair_id0"], j["pes_in"], psel_cap)


def same(got, want):
    """Byte-exact on the estimate, the pair records, the regions, the count and the new list with its tail; names the first
    difference."""
    assert got["n_psel"] == want["n_psel"], (got["n_psel"], want["n_psel"])
    for k in ("pes", "pairs", "pregs"):
        g, w = got[k], want[k]
        assert g.dtype == w.dtype and len(g) == len(w), k
        for f in w.dtype.names:
            bad = np.nonzero(g[f] != w[f])[0]
            assert len(bad) == 0, "%s.%s differs at %s: %s != %s" % (k, f, bad[:5], g[f][bad[:5]], w[f][bad[:5]])
        assert g.tobytes() == w.tobytes(), k
    for k in ("psel_seeds", "psel_res"):
        assert got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), k


def example():
    with open(os.path.join(HERE, "golden", "mem_pair_example.json")) as f:
        return json.load(f)
