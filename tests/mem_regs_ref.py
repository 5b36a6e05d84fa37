"""Plain-Python restatement of the alignment-region rules (include/gbx.h "alignment regions"): the redundancy skip
of bwa-mem's mem_chain2aln, mem_sort_dedup_patch without mem_patch_reg, mem_mark_primary_se, mem_approx_mapq_se and the region
choice of mem_reg2sam, as the gbx_mem_regs_* entries are specified.  Serial, step by step; no device code and nothing shared
with genomicsbench_amd.mem_regs.

mapq and the last bit of log(): every mapq is computed with each of its two logarithms as the C library gives it and moved one
ulp down and up, independently (nine values).  A region where they are not all equal is a boundary input: `boundary` in the
result counts them, and the tests require that their inputs hold none, so that a device log() that differs in the last bit
cannot change a byte.
"""
import math

import numpy as np

from mem_chain_ref import CHAIN_DTYPE, SEED_DTYPE

RESULT_FIELDS = ("score", "truesc", "qb", "qe", "rb", "re", "w", "sc0")
REG_DTYPE = np.dtype([("rb", "<i8"), ("re", "<i8"), ("seed", "<i8"), ("qb", "<i4"), ("qe", "<i4"), ("read", "<i4"), ("rid", "<i4"),
                      ("score", "<i4"), ("truesc", "<i4"), ("sub", "<i4"), ("sub_n", "<i4"), ("w", "<i4"), ("seedcov", "<i4"),
                      ("seedlen0", "<i4"), ("secondary", "<i4"), ("mapq", "<i4"), ("flag", "<i4"), ("sel", "<i4"), ("pad_", "<i4")])
assert REG_DTYPE.itemsize == 88
DEFAULTS = dict(a=1, b=4, o_del=6, e_del=1, o_ins=6, e_ins=1, w=100, max_chain_gap=10000, min_seed_len=19, T=30, mapq_coef_len=50,
                mapq_coef_fac=float(np.float32(math.log(50.0))), mask_level=0.5, mask_level_redun=0.95, drop_ratio=0.5)
M64 = (1 << 64) - 1
f32 = np.float32


def params(**kw):
    p = dict(DEFAULTS)
    for k in kw:
        assert k in p, k
    p.update(kw)
    if "mapq_coef_len" in kw and "mapq_coef_fac" not in kw:
        p["mapq_coef_fac"] = float(np.float32(math.log(float(p["mapq_coef_len"]))))
    return p


def hash_64(k):
    k &= M64
    k = (k + (~(k << 32) & M64)) & M64
    k ^= k >> 22
    k = (k + (~(k << 13) & M64)) & M64
    k ^= k >> 8
    k = (k + (k << 3)) & M64
    k ^= k >> 15
    k = (k + (~(k << 27) & M64)) & M64
    k ^= k >> 31
    return k


def gap(q, P):
    """The window function of DESIGN 3.10 (bwa's cal_max_gap)."""
    gd = int((q * P["a"] - P["o_del"]) / P["e_del"] + 1.)
    gi = int((q * P["a"] - P["o_ins"]) / P["e_ins"] + 1.)
    return min(max(max(gd, gi), 1), 2 * P["w"])


class Seed:
    def __init__(self, idx, k, s, r):
        self.idx, self.k = idx, k                    # its record's index; its index in the chain
        self.qbeg, self.len, self.lq, self.roff = int(s["qbeg"]), int(s["len"]), int(s["lq"]), int(s["roff"])
        self.rbeg = self.roff + int(s["rbeg"])       # absolute
        self.res = {f: int(r[i]) for i, f in enumerate(RESULT_FIELDS)}
        self.present = self.res["qb"] >= 0
        self.took = False


class Reg:
    def __init__(self, s, rid):
        e = s.res
        self.rb, self.re, self.qb, self.qe = s.roff + e["rb"], s.roff + e["re"], e["qb"], e["qe"]
        self.score, self.truesc, self.w = e["score"], e["truesc"], e["w"]
        self.seedlen0, self.rid, self.seed, self.roff, self.lq = s.len, rid, s.idx, s.roff, s.lq
        self.seedcov = self.sub = self.sub_n = self.mapq = self.flag = 0
        self.secondary = self.sel = -1
        self.excluded = False


def around(s, p, P):
    """The seed lies inside region p on both axes, is not much longer than p's seed, and is near p's diagonal ahead or behind."""
    if s.rbeg < p.rb or s.rbeg + s.len > p.re or s.qbeg < p.qb or s.qbeg + s.len > p.qe:
        return False
    if s.len - p.seedlen0 > .1 * s.lq:
        return False
    qd, rd = s.qbeg - p.qb, s.rbeg - p.rb
    wg = min(gap(min(qd, rd), P), p.w)
    if qd - rd < wg and rd - qd < wg:
        return True
    qd, rd = p.qe - (s.qbeg + s.len), p.re - (s.rbeg + s.len)
    wg = min(gap(min(qd, rd), P), p.w)
    return qd - rd < wg and rd - qd < wg


def choose(chains, P):
    """Step 1.  chains: [(contig, [Seed, ...]), ...] of one read -> av, the regions in creation order."""
    av = []
    for rid, seeds in chains:
        order = sorted((s for s in seeds if s.present), key=lambda s: (s.len, s.k), reverse=True)
        for s in order:
            stopped = any(around(s, p, P) for p in av)          # (the first such p ends bwa's scan; the scan has no side effect)
            if stopped:
                rescued = False
                for t in seeds:
                    if not t.took or t.len < s.len * .95:
                        continue
                    # the mirrored test keeps s.len >> 2, as bwa's source does
                    if s.qbeg <= t.qbeg and s.qbeg + s.len - t.qbeg >= s.len >> 2 and t.qbeg - s.qbeg != t.rbeg - s.rbeg:
                        rescued = True
                    if t.qbeg <= s.qbeg and t.qbeg + t.len - s.qbeg >= s.len >> 2 and s.qbeg - t.qbeg != s.rbeg - t.rbeg:
                        rescued = True
                if not rescued:
                    continue
            a = Reg(s, rid)
            a.seedcov = sum(t.len for t in seeds if t.present and t.qbeg >= a.qb and t.qbeg + t.len <= a.qe and t.rbeg >= a.rb and
                            t.rbeg + t.len <= a.re)
            s.took = True
            av.append(a)
    return av


def dedup(av, P):
    """Step 2: mem_sort_dedup_patch; the branch through mem_patch_reg is not modelled."""
    if len(av) < 2:
        return list(av)
    a = [x for _, x in sorted(enumerate(av), key=lambda t: (t[1].re, t[0]))]
    mlr = f32(P["mask_level_redun"])
    for i in range(1, len(a)):
        p = a[i]
        j = i - 1
        while j >= 0 and a[j].rid == p.rid and p.rb < a[j].re + P["max_chain_gap"]:
            q = a[j]
            j -= 1
            if q.excluded:
                continue
            orr = q.re - p.rb
            oq = q.qe - p.qb if q.qb < p.qb else p.qe - q.qb
            mr, mq = min(q.re - q.rb, p.re - p.rb), min(q.qe - q.qb, p.qe - p.qb)
            if f32(orr) > mlr * f32(mr) and f32(oq) > mlr * f32(mq):
                if p.score < q.score:
                    p.excluded = True
                    break
                q.excluded = True
    a = [x for x in a if not x.excluded]
    a = [x for _, x in sorted(enumerate(a), key=lambda t: (-t[1].score, t[1].rb, t[1].qb, t[0]))]
    for i in range(1, len(a)):
        if a[i].score == a[i - 1].score and a[i].rb == a[i - 1].rb and a[i].qb == a[i - 1].qb:
            a[i].excluded = True
    return [x for x in a if not x.excluded]


def mark_primary(a, read_id, P):
    """Step 3 -> the regions in output order, secondary / sub / sub_n set."""
    for i, x in enumerate(a):
        x.sub = x.sub_n = 0
        x.secondary = -1
        x.hash = hash_64(read_id + i)
    a = [x for _, x in sorted(enumerate(a), key=lambda t: (-t[1].score, t[1].hash, t[0]))]
    if not a:
        return a
    tmp = max(P["a"] + P["b"], P["o_del"] + P["e_del"], P["o_ins"] + P["e_ins"])
    ml = f32(P["mask_level"])
    z = [0]
    for i in range(1, len(a)):
        for j in z:
            b_max, e_min = max(a[j].qb, a[i].qb), min(a[j].qe, a[i].qe)
            if e_min > b_max:
                min_l = min(a[i].qe - a[i].qb, a[j].qe - a[j].qb)
                if f32(e_min - b_max) >= f32(min_l) * ml:
                    if a[j].sub == 0:
                        a[j].sub = a[i].score
                    if a[j].score - a[i].score <= tmp:
                        a[j].sub_n += 1
                    a[i].secondary = j
                    break
        else:
            z.append(i)
    return a


def _ulps(x):
    return (x, math.nextafter(x, -math.inf), math.nextafter(x, math.inf))


def mapq_values(x, l_rep, P):
    """Step 4 -> the mapq with each logarithm as it is and one ulp down / up (a list; all equal off a boundary)."""
    sub = x.sub if x.sub else P["min_seed_len"] * P["a"]
    if sub >= x.score:
        return [0]
    l = max(x.qe - x.qb, x.re - x.rb)
    if l < 1 or x.score == 0:                        # (l < 1 cannot come out of an extension; it would divide by zero)
        return [0]
    identity = 1. - float(l * P["a"] - x.score) / float(P["a"] + P["b"]) / float(l)
    frac_rep = f32(l_rep) / f32(x.lq)
    out = []
    for lg_l in (_ulps(math.log(float(l))) if l >= P["mapq_coef_len"] else (None,)):
        for lg_n in (_ulps(math.log(float(x.sub_n + 1))) if x.sub_n > 0 else (None,)):
            t = 1. if lg_l is None else float(f32(P["mapq_coef_fac"])) / lg_l
            t *= identity * identity
            mapq = int(6.02 * float(x.score - sub) / float(P["a"]) * t * t + .499)
            if lg_n is not None:
                mapq -= int(4.343 * lg_n + .499)
            mapq = max(0, min(60, mapq))
            out.append(int(float(mapq) * (1. - float(frac_rep)) + .499))
    return out


def report(a, l_rep, P):
    """Steps 4 and 5 -> (number reported, number of boundary inputs)."""
    boundary = 0
    for x in a:
        x.mapq = 0
        if x.secondary < 0:
            v = mapq_values(x, l_rep, P)
            boundary += len(set(v)) > 1
            x.mapq = v[0]
    l = 0
    first = None
    for x in a:
        x.flag, x.sel = 0, -1
        if x.score < P["T"]:
            continue
        if x.secondary >= 0:
            continue
        if x.secondary >= 0 and f32(x.score) < f32(a[x.secondary].score) * f32(P["drop_ratio"]):      # dead under the line above
            continue
        x.flag = 1
        if l > 0:
            x.flag |= 0x800
            x.mapq = min(x.mapq, first.mapq)
        else:
            first = x
        x.sel = l
        l += 1
    return l, boundary


def regs_all(chains, chain_off, seeds, res, l_rep, P=None, read_id0=0, sel_cap=None, detail=None):
    """Every read -> dict(regs REG_DTYPE, reg_off, n_regs, sel_seeds SEED_DTYPE[sel_cap], sel_res int32[sel_cap, 8], n_sel,
    boundary).  sel_cap defaults to the number of seeds; the CIGAR list past n_sel is zeroed seeds with results of all -1.
    detail: a list that receives, per read, dict(made, after_dedup) with the seed indices of the regions at those points."""
    P = P or params()
    chains = np.asarray(chains, dtype=CHAIN_DTYPE)
    seeds = np.asarray(seeds, dtype=SEED_DTYPE)
    res = np.ascontiguousarray(res, dtype=np.int32).reshape(-1, 8)
    n_reads = len(chain_off) - 1
    sel_cap = len(seeds) if sel_cap is None else sel_cap
    regs, reg_off, sel, boundary = [], [0], [], 0
    for r in range(n_reads):
        mine = []
        for c in range(int(chain_off[r]), int(chain_off[r + 1])):
            so, ns = int(chains[c]["seed_off"]), int(chains[c]["n_seeds"])
            mine.append((int(chains[c]["contig"]), [Seed(so + k, k, seeds[so + k], res[so + k]) for k in range(ns)]))
        av = choose(mine, P)
        a = dedup(av, P)
        if detail is not None:
            detail.append(dict(made=[x.seed for x in av], after_dedup=[x.seed for x in a]))
        a = mark_primary(a, read_id0 + r, P)
        _, b = report(a, int(l_rep[r]), P)
        boundary += b
        for x in a:
            if x.flag & 1:
                x.sel = len(sel)
                sel.append(x)
            regs.append((x.rb, x.re, x.seed, x.qb, x.qe, r, x.rid, x.score, x.truesc, x.sub, x.sub_n, x.w, x.seedcov, x.seedlen0,
                         x.secondary, x.mapq, x.flag, x.sel, 0))
        reg_off.append(len(regs))
    sel_seeds = np.zeros(sel_cap, dtype=SEED_DTYPE)
    sel_res = np.full((sel_cap, 8), -1, dtype=np.int32)
    for k, x in enumerate(sel[:sel_cap]):
        sel_seeds[k] = seeds[x.seed]
        sel_res[k] = (x.score, x.truesc, x.qb, x.qe, x.rb - x.roff, x.re - x.roff, x.w, 0)
    return dict(regs=np.array(regs, dtype=REG_DTYPE), reg_off=np.array(reg_off, dtype=np.int64), n_regs=len(regs),
                sel_seeds=sel_seeds, sel_res=sel_res, n_sel=len(sel), boundary=boundary)
