"""Inputs of the alignment-region tests (gbx_mem_regs_*), shared by the CPU and the GPU tests: hand-built reads, one per rule and
per branch of the specification with the outcome written out by hand, and generators of reads whose chains, seeds
and extension results are made up (no index, no extension), among them reads built to straddle the wave width.

A job is dict(params, read_id0, chains CHAIN_DTYPE, chain_off, seeds SEED_DTYPE, res int32[n, 8], l_rep); a hand-built job has
`expect` as well: per read (made, out) - the seed records that made a region in step 1, in creation order, and the regions
in output order as (seed, secondary, sub, sub_n, seedcov, mapq, flag, sel)."""
import functools
import json
import os

import numpy as np

import mem_regs_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


class Builder:
    def __init__(self, read_id0=0, **params):
        self.params, self.read_id0 = params, read_id0
        self.chains, self.chain_off, self.seeds, self.res, self.l_rep, self.qoff = [], [0], [], [], [], 0

    def read(self, lq, chains, l_rep=0):
        """chains: [(contig, roff, rlen, [(qbeg, len, rbeg, result), ...]), ...] with absolute rbeg; result: None (the
        extension's all -1) or (qb, qe, rb, re, score[, w[, truesc]]) with absolute rb / re."""
        r = len(self.l_rep)
        for contig, roff, rlen, sds in chains:
            self.chains.append((sds[0][2] if sds else 0, len(self.seeds), roff, roff + rlen, r, contig, len(sds), 0, 3, 0))
            for q, ln, rabs, e in sds:
                self.seeds.append((self.qoff, roff, lq, rlen, q, rabs - roff, ln, 0))
                if e is None:
                    self.res.append((-1,) * 8)
                else:
                    qb, qe, rb, re, sc = e[:5]
                    w = e[5] if len(e) > 5 else 100
                    self.res.append((sc, e[6] if len(e) > 6 else sc, qb, qe, rb - roff, re - roff, w, 7))
        self.chain_off.append(len(self.chains))
        self.l_rep.append(l_rep)
        self.qoff += lq

    def job(self, expect=None):
        j = dict(params=self.params, read_id0=self.read_id0, chains=np.array(self.chains, dtype=R.CHAIN_DTYPE),
                 chain_off=np.array(self.chain_off, dtype=np.int64), seeds=np.array(self.seeds, dtype=R.SEED_DTYPE),
                 res=np.array(self.res, dtype=np.int32).reshape(-1, 8), l_rep=np.array(self.l_rep, dtype=np.int32))
        if expect is not None:
            j["expect"] = expect
        return j


WHOLE = (0, 100, 1000, 1100, 100)                     # a 100-base read aligned end to end at 1000


def one(chains, expect, lq=100, l_rep=0, **params):
    b = Builder(**params)
    b.read(lq, chains, l_rep)
    return b.job([expect])


@functools.lru_cache(maxsize=None)
def hand_built():
    """name -> job.  lq = 100, bwa's scoring: a perfect end-to-end hit has mapq 60; tmp = max(a + b, o + e) = 7."""
    J = {}
    # B lies inside A's region on A's diagonal, 60 bases ahead (gap(60) = 55): no region; seedcov counts both seeds
    J["inside_skipped"] = one([(0, 900, 400, [(0, 50, 1000, WHOLE), (60, 30, 1060, WHOLE)])], ([0], [(0, -1, 0, 0, 80, 60, 1, 0)]))
    # a second chain's seed inside the first region: 31 - 20 > .1 lq keeps it (its own region then loses the dedup on a
    # tie: the earlier one, q, goes); 30 - 20 = 10 does not, and the chain has no taken seed to rescue it
    b = Builder()
    b.read(100, [(0, 900, 400, [(40, 20, 1040, WHOLE)]), (0, 900, 400, [(10, 31, 1010, WHOLE)])])
    b.read(100, [(0, 900, 400, [(40, 20, 1040, WHOLE)]), (0, 900, 400, [(10, 30, 1010, WHOLE)])])
    J["tenth_of_lq"] = b.job([([0, 1], [(1, -1, 0, 0, 31, 60, 1, 0)]), ([2], [(2, -1, 0, 0, 20, 60, 1, 1)])])
    # two seeds of one chain, 10 = 40 >> 2 bases of overlap, diagonals 2 apart: the second one taken is rescued, whichever
    # comes first on the query; with 9 bases of overlap it is not
    wide = (0, 100, 1000, 1102, 92)
    b = Builder()
    b.read(100, [(0, 900, 400, [(0, 40, 1000, (0, 100, 1000, 1102, 90)), (30, 40, 1032, wide)])])          # s before t
    b.read(100, [(0, 900, 400, [(30, 40, 1032, (0, 100, 1000, 1102, 90)), (0, 40, 1000, wide)])])          # t before s
    b.read(100, [(0, 900, 400, [(31, 40, 1033, (0, 100, 1000, 1102, 90)), (0, 40, 1000, wide)])])          # 9 bases
    J["overlapping_seed"] = b.job([([1, 0], [(1, -1, 0, 0, 80, 60, 1, 0)]), ([3, 2], [(3, -1, 0, 0, 80, 60, 1, 1)]),
                                   ([5], [(5, -1, 0, 0, 80, 60, 1, 2)])])
    # dedup: X = q[0, 90) r[1000, 1090), then Z = q[2, 100) r[1002, 1100) from a seed that pokes out of X; 88 > .95 * 90 on
    # both axes.  Z is p (the larger re): lower score - p goes; higher or equal - q goes
    def xz(sx, sz, mid=None, **params):
        chains = [(0, 900, 400, [(0, 30, 1000, (0, 90, 1000, 1090, sx))])]
        if mid is not None:                                                      # W = q[40, 70) r[1030, 1095) between them
            chains.append((mid, 900, 400, [(45, 4, 1091, (40, 70, 1030, 1095, 30))]))
        chains.append((0, 900, 400, [(85, 15, 1085, (2, 100, 1002, 1100, sz))]))
        return chains
    b = Builder()
    b.read(100, xz(90, 80))
    b.read(100, xz(90, 95))
    b.read(100, xz(90, 90))
    J["dedup"] = b.job([([0, 1], [(0, -1, 0, 0, 30, 60, 1, 0)]), ([2, 3], [(3, -1, 0, 0, 15, 60, 1, 1)]),
                        ([4, 5], [(5, -1, 0, 0, 15, 60, 1, 2)])])
    # the j walk: W (score 30) between X and Z.  Same contig: the walk excludes W (it lies inside Z), goes on and excludes X.  W
    # on another contig: the walk ends at W, all three stay, X and W secondary to Z (95 - 90 <= tmp: sub_n 1; mapq 21 - 3).
    # max_chain_gap = -90: W is passed and excluded (1002 < 1095 - 90), X ends the walk (1002 < 1090 - 90 is false) and stays
    b = Builder()
    b.read(100, xz(90, 95, mid=0))
    b.read(100, xz(90, 95, mid=1))
    J["walk_rid"] = b.job([([0, 1, 2], [(2, -1, 0, 0, 15, 60, 1, 0)]),
                           ([3, 4, 5], [(5, -1, 90, 1, 15, 18, 1, 1), (3, 0, 0, 0, 30, 0, 0, -1), (4, 0, 0, 0, 4, 0, 0, -1)])])
    b = Builder(max_chain_gap=-90)
    b.read(100, xz(90, 95, mid=0))
    J["walk_max_chain_gap"] = b.job([([0, 1, 2], [(2, -1, 90, 1, 15, 18, 1, 0), (0, 0, 0, 0, 30, 0, 0, -1)])])
    # two hits equal in score, rb and qb on two contigs (the walk ends at the rid, so the first pass keeps both; the second
    # one's seed pokes out of the first region, so step 1 makes it): the second one of the (score, rb, qb, previous index) order
    # goes, and the shorter hit is the earlier one there, having the smaller re
    J["identical_hit"] = one([(0, 900, 400, [(0, 30, 1000, (0, 100, 1000, 1100, 50))]), (1, 900, 400, [(5, 10, 1095, (0, 40, 1000, 1040, 50))])],
                             ([0, 1], [(1, -1, 0, 0, 0, 60, 1, 0)]))
    # three hits of the whole read at three loci, 100 / 96 / 90: sub is set once (96), sub_n counts the one within tmp = 7
    J["secondary"] = one([(0, 900, 400, [(0, 30, 1000, WHOLE)]), (0, 4900, 400, [(0, 30, 5000, (0, 100, 5000, 5100, 96))]),
                          (0, 8900, 400, [(0, 30, 9000, (0, 100, 9000, 9100, 90))])],
                         ([0, 1, 2], [(0, -1, 96, 1, 30, 14, 1, 0), (1, 0, 0, 0, 30, 0, 0, -1), (2, 0, 0, 0, 30, 0, 0, -1)]))
    # q[0, 50) at one locus (50, and 48 at a third locus beneath it: mapq 9), q[50, 100) at another (45, alone: mapq 60):
    # the second is supplementary and its mapq is capped by the first's
    J["supplementary"] = one([(0, 900, 400, [(0, 30, 1000, (0, 50, 1000, 1050, 50))]), (0, 4900, 400, [(50, 30, 5050, (50, 100, 5050, 5100, 45))]),
                              (0, 8900, 400, [(0, 30, 9000, (0, 50, 9000, 9050, 48))])],
                             ([0, 1, 2], [(0, -1, 48, 1, 30, 9, 1, 0), (2, 0, 0, 0, 30, 0, 0, -1), (1, -1, 0, 0, 30, 9, 0x801, 1)]))
    # score 25 < T: a region with a mapq, not reported
    J["below_T"] = one([(0, 900, 400, [(0, 25, 1000, (0, 25, 1000, 1025, 25))])], ([0], [(0, -1, 0, 0, 25, 36, 0, -1)]))
    J["below_T_lowered"] = one([(0, 900, 400, [(0, 25, 1000, (0, 25, 1000, 1025, 25))])], ([0], [(0, -1, 0, 0, 25, 36, 1, 0)]), T=20)
    # l_rep = 30 of 100 bases: 60 * (1 - 0.3f) + .499 -> 42
    J["frac_rep"] = one([(0, 900, 400, [(0, 50, 1000, WHOLE)])], ([0], [(0, -1, 0, 0, 50, 42, 1, 0)]), l_rep=30)
    # a seed the extension answered with all -1: no region from it, not in seedcov; a chain of nothing else makes nothing
    b = Builder()
    b.read(100, [(0, 900, 400, [(0, 60, 1000, None), (70, 30, 1070, WHOLE)]), (0, 4900, 400, [(0, 30, 5000, None)])])
    b.read(100, [])                                                              # a read with no chains
    b.read(100, [(0, 900, 400, [(0, 50, 1000, WHOLE)])])
    J["absent_and_empty"] = b.job([([1], [(1, -1, 0, 0, 30, 60, 1, 0)]), ([], []), ([3], [(3, -1, 0, 0, 50, 60, 1, 1)])])
    # other scoring and another read_id0 (the hash decides between equal scores): tmp = max(2 + 3, 5 + 2, 4 + 1) = 7 < 200 - 192
    b = Builder(read_id0=1234567, a=2, b=3, o_del=5, e_del=2, o_ins=4, e_ins=1, min_seed_len=10, T=40)
    b.read(100, [(0, 900, 400, [(0, 30, 1000, (0, 100, 1000, 1100, 200))]), (0, 4900, 400, [(0, 30, 5000, (0, 100, 5000, 5100, 200))]),
                 (0, 8900, 400, [(0, 30, 9000, (0, 100, 9000, 9100, 192))])])
    J["scoring"] = b.job([([0, 1, 2], [(1, -1, 200, 1, 30, 0, 1, 0), (0, 0, 0, 0, 30, 0, 0, -1), (2, 0, 0, 0, 30, 0, 0, -1)])])
    return J


def many_regions(b, n, rng, lq=None, slots=True, contig_of=lambda i: 0):
    """One read of n single-seed chains at loci 1000 apart.  slots: disjoint query slots of 40 bases (n primaries, so z grows to
    n); otherwise random spans of the read (primaries and secondaries)."""
    lq = lq or max(100, 40 * n)
    chains = []
    for i in range(n):
        if slots:
            qb, qe = 40 * i, 40 * i + 40
        else:
            qb = int(rng.integers(0, lq - 40))
            qe = qb + int(rng.integers(30, lq - qb + 1))
        roff = 1000 + 8000 * i
        rb = roff + 100 + qb
        sc = int(rng.integers(20, qe - qb + 1))
        q = int(rng.integers(qb, qe - 9))
        chains.append((contig_of(i), roff, 7000, [(q, min(10, qe - q), rb + q - qb, (qb, qe, rb, rb + qe - qb + int(rng.integers(-2, 3)), sc))]))
    b.read(lq, chains, l_rep=int(rng.integers(0, 20)))


def long_chain(b, n, rng, lq=400):
    """One read with one chain of n seeds on three close diagonals, whose results are a handful of nearly equal regions: most
    seeds are skipped, some are rescued by the overlapping-seed clause, the regions they make meet in the dedup."""
    roff, sds = 5000, []
    variants = [(0, lq, 5100, 5100 + lq, lq - 20), (0, lq - 3, 5100, 5097 + lq, lq - 24), (4, lq, 5105, 5101 + lq, lq - 26),
                (0, lq // 2, 5100, 5100 + lq // 2, lq // 2 - 5)]
    for i in range(n):
        q = int(rng.integers(0, lq - 40))
        ln = int(rng.integers(19, 40))
        d = int(rng.integers(0, 3))
        e = variants[int(rng.integers(0, len(variants)))] if rng.random() > 0.05 else None
        sds.append((q, ln, 5100 + q + d, e))
    b.read(lq, [(0, roff, 1000, sds)], l_rep=int(rng.integers(0, 30)))


def loci_read(b, rng, lq=151):
    """A read as the pipeline makes them: a few loci, per locus a chain of collinear seeds whose results are small variations of
    one region (what the extension finds from different seeds), some partial, some absent."""
    chains = []
    for _ in range(int(rng.integers(0, 5))):
        roff = int(rng.integers(0, 40)) * 3000
        base = roff + 300
        qb0, qe0 = int(rng.integers(0, 30)) * int(rng.random() < 0.5), lq - int(rng.integers(0, 30)) * int(rng.random() < 0.5)
        cut = int(rng.integers(50, lq - 50))
        kind = rng.random()
        if kind < 0.2:                                                           # the read's left or right part only
            qe0 = cut
        elif kind < 0.4:
            qb0 = cut
        top = int(rng.integers(20, qe0 - qb0 + 1))
        sds = []
        q = qb0
        while q < qe0 - 19:
            ln = int(rng.integers(19, min(60, qe0 - q) + 1))
            if rng.random() < 0.85:
                d = int(rng.integers(-2, 3)) * int(rng.random() < 0.3)
                if rng.random() < 0.08:
                    e = None
                else:
                    qb = qb0 + int(rng.integers(0, 12)) * int(rng.random() < 0.3)
                    qe = qe0 - int(rng.integers(0, 12)) * int(rng.random() < 0.3)
                    e = (qb, qe, base + qb, base + qe + d, max(1, top - int(rng.integers(0, 9)) * int(rng.random() < 0.5)),
                         int(rng.integers(1, 101)))
                sds.append((q, ln, base + q + d, e))
            q += int(rng.integers(5, 50))
        if sds:
            chains.append((int(roff >= 60000), roff, 1000, sds))
    b.read(lq, chains, l_rep=int(rng.integers(0, 40)) * int(rng.random() < 0.3))


def synthetic(n_reads, seed, read_id0=0, **params):
    rng = np.random.default_rng(seed)
    b = Builder(read_id0=read_id0, **params)
    for _ in range(n_reads):
        loci_read(b, rng)
    return b.job()


def straddle(seed=4):
    """Reads of 0, 1, 2, 63, 64, 65 and 130 regions (the last one all primaries: z passes 64 entries), 70 and 130 overlapping
    ones, chains of 100 and 200 seeds, one read with regions on two contigs."""
    rng = np.random.default_rng(seed)
    b = Builder(read_id0=99)
    for n in (0, 1, 2, 63, 64, 65, 130):
        many_regions(b, n, rng)
    for n in (70, 130):
        many_regions(b, n, rng, lq=300, slots=False, contig_of=lambda i: i % 2)
    for n in (100, 200):
        long_chain(b, n, rng)
    return b.job()


def p_of(j):
    return R.params(**j["params"])


def reference(j, sel_cap=None, detail=None):
    if sel_cap is None and detail is None:            # computed once per job, shared and left unchanged by its users
        if "_ref" not in j:
            j["_ref"] = R.regs_all(j["chains"], j["chain_off"], j["seeds"], j["res"], j["l_rep"], p_of(j), j["read_id0"])
        return j["_ref"]
    return R.regs_all(j["chains"], j["chain_off"], j["seeds"], j["res"], j["l_rep"], p_of(j), j["read_id0"], sel_cap, detail)


def same(got, want, sel_cap=None):
    """Byte-exact on regs, reg_off, the counts and the CIGAR list with its tail; names the first difference."""
    assert got["n_regs"] == want["n_regs"] and got["n_sel"] == want["n_sel"], (got["n_regs"], got["n_sel"], want["n_regs"], want["n_sel"])
    assert np.array_equal(got["reg_off"], want["reg_off"])
    g, w = got["regs"], want["regs"]
    assert g.dtype == w.dtype and len(g) == len(w)
    for f in w.dtype.names:
        bad = np.nonzero(g[f] != w[f])[0]
        assert len(bad) == 0, "field %s differs at regions %s: %s != %s" % (f, bad[:5], g[f][bad[:5]], w[f][bad[:5]])
    assert g.tobytes() == w.tobytes()
    for k in ("sel_seeds", "sel_res"):
        assert got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), k


def example():
    with open(os.path.join(HERE, "golden", "mem_regs_example.json")) as f:
        return json.load(f)
