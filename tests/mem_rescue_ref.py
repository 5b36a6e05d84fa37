"""Plain-Python restatement of the mate-rescue rules (include/gbx.h "mate rescue"): bwa-mem's mem_matesw around
ksw_align2, as the gbx_mem_rescue_* entries are specified, and the insert-size estimate alone (gbx_mem_pestat_*).  Serial, step by
step; no device code and nothing shared with genomicsbench_amd.mem_rescue.  dedup and mark_primary are those of mem_regs_ref, the
estimate is that of mem_pair_ref; the mapq and report rules are restated here because they change: a region carries csub, and a
region with seedlen0 == 0 has frac_rep = 0.

Boundary inputs are counted the way mem_regs_ref.report counts them: every mapq is computed with each of its two logarithms as
the C library gives it and one ulp down and up; a region where the nine values are not all equal is a boundary input.
"""
import math

import numpy as np

import mem_pair_ref as PR
import mem_regs_ref as RG
from mem_regs_ref import SEED_DTYPE, f32

REG_DTYPE = np.dtype([(n if n != "pad_" else "csub", t) for n, t in RG.REG_DTYPE.descr])
STAT_DTYPE = np.dtype([("n_sw", "<i4"), ("n_added", "<i4"), ("n_kept", "<i4"), ("pad_", "<i4")])
PESTAT_DTYPE = PR.PESTAT_DTYPE
assert REG_DTYPE.itemsize == 88 and STAT_DTYPE.itemsize == 16
DEFAULTS = dict(a=1, b=4, o_del=6, e_del=1, o_ins=6, e_ins=1, min_seed_len=19, T=30, pen_unpaired=17, max_matesw=50,
                max_chain_gap=10000, mask_level=0.5, mask_level_redun=0.95, mapq_coef_len=50,
                mapq_coef_fac=float(np.float32(math.log(50.0))))
PAD = 5                                              # the symbol that fills the query up to slen * Pw rows: 0 against everything


def params(**kw):
    p = dict(DEFAULTS)
    for k in kw:
        assert k in p, k
    p.update(kw)
    if "mapq_coef_len" in kw and "mapq_coef_fac" not in kw:
        p["mapq_coef_fac"] = float(np.float32(math.log(float(p["mapq_coef_len"]))))
    return p


# ---- rule 3: the SW
def lanes_of(m, P):
    return 16 if m * P["a"] < 250 else 8


def sw_pass(q, t, P, Pw, endsc=None):
    """One pass of ksw_align2's kernel -> (score, te, qe, entries).  q along the rows, padded to slen * Pw rows; t along the
    columns.  endsc: the pass stops at the first column where gmax >= endsc and makes no entries."""
    a, b = P["a"], P["b"]
    oe_d, e_d, oe_i, e_i = P["o_del"] + P["e_del"], P["e_del"], P["o_ins"] + P["e_ins"], P["e_ins"]
    minsc = P["min_seed_len"] * a
    m, n = len(q), len(t)
    slen = (m + Pw - 1) // Pw
    mp = slen * Pw
    qq = np.full(mp, PAD, dtype=np.int64)
    qq[:m] = q
    prof = np.zeros((5, mp), dtype=np.int64)
    for y in range(5):
        prof[y] = np.where(qq == PAD, 0, np.where((qq > 3) | (y > 3), -1, np.where(qq == y, a, -b)))
    j = np.arange(mp, dtype=np.int64)
    key = (j % slen) * Pw + j // slen                # a row's place in striped memory
    H = np.zeros(mp, dtype=np.int64)
    E = np.zeros(mp, dtype=np.int64)
    F = np.zeros(mp, dtype=np.int64)
    diag = np.zeros(mp, dtype=np.int64)
    gmax, te, h_te, ents = 0, -1, None, []
    for i in range(n):
        diag[1:] = H[:-1]
        h0 = np.maximum(0, np.maximum(diag + prof[min(int(t[i]), 4)], E))
        # F(i, j + 1) = max(0, F(i, j) - e_ins, H(i, j) - o_ins - e_ins) unrolled: the largest h0[k] - oe - e (j - k) over k <= j
        run = np.maximum.accumulate(h0 - oe_i + e_i * j)
        F[1:] = np.maximum(0, run[:-1] - e_i * j[:-1])
        H = np.maximum(h0, F)
        E = np.maximum(0, np.maximum(E - e_d, H - oe_d))
        imax = int(H.max())
        if endsc is None and imax >= minsc:
            if not ents or ents[-1][1] + 1 != i:
                ents.append((imax, i))
            elif ents[-1][0] < imax:
                ents[-1] = (imax, i)
        if imax > gmax:
            gmax, te, h_te = imax, i, H.copy()
            if endsc is not None and gmax >= endsc:
                break
    qe = -1
    if te >= 0:
        rows = np.nonzero(h_te == gmax)[0]
        qe = int(rows[np.argmin(key[rows])])
        assert qe < m
    return gmax, te, qe, ents


def sw(q, t, P):
    """ksw_align2 with KSW_XSUBO | KSW_XSTART | min_seed_len * a -> (score, te, qe, score2, te2, qb, tb)."""
    q, t = np.asarray(q, dtype=np.int64), np.asarray(t, dtype=np.int64)
    a = P["a"]
    Pw = lanes_of(len(q), P)
    score, te, qe, ents = sw_pass(q, t, P, Pw)
    w = (score + a - 1) // a
    score2, te2 = -1, -1
    for v, c in ents:
        if (c < te - w or c > te + w) and v > score2:
            score2, te2 = v, c
    if score < P["min_seed_len"] * a:
        return score, te, qe, score2, te2, -1, -1
    s1, te1, qe1, _ = sw_pass(q[:qe + 1][::-1], t[:te + 1][::-1], P, Pw, endsc=score)
    assert s1 == score, (s1, score)
    return score, te, qe, score2, te2, qe - qe1, te - te1


# ---- rules 0 to 2
class Reg:
    FIELDS = REG_DTYPE.names

    def __init__(self, row=None):
        for f in self.FIELDS:
            setattr(self, f, int(row[f]) if row is not None else 0)
        self.excluded = False
        self.lq = 0
        self.win = None                              # a rescued region: (roff, rlen) of its seed record

    def row(self):
        return tuple(getattr(self, f) for f in self.FIELDS)


def revcomp(s):
    s = np.asarray(s)
    return np.where(s < 4, 3 - s, 4)[::-1]


def window(anchor, r, pe, l_ms, L, contig_off, P):
    """The window of direction r around the anchor -> (rb, re, is_rev) or None."""
    low, high = pe[0], pe[1]
    is_rev = (r >> 1) != (r & 1)
    is_larger = not (r >> 1)
    if not is_rev:
        rb = anchor.rb + low if is_larger else anchor.rb - high
        re = (anchor.rb + high if is_larger else anchor.rb - low) + l_ms
    else:
        rb = (anchor.rb + low if is_larger else anchor.rb - high) - l_ms
        re = anchor.rb + high if is_larger else anchor.rb - low
    rb, re = max(rb, 0), min(re, 2 * L)
    if rb >= re:
        return None
    mid = (rb + re) >> 1
    rev = mid >= L
    fwd = 2 * L - 1 - mid if rev else mid
    rid = int(np.searchsorted(contig_off, fwd, side="right") - 1)
    c0, c1 = int(contig_off[rid]), int(contig_off[rid + 1])
    lo, hi = (2 * L - c1, 2 * L - c0) if rev else (c0, c1)
    rb, re = max(rb, lo), min(re, hi)
    if rid != anchor.rid or re - rb < P["min_seed_len"]:
        return None
    return rb, re, is_rev


def matesw(anchor, mate, ma, pes, L, contig_off, text, P):
    """One call of mem_matesw; ma is changed in place -> (SWs run, regions added)."""
    skip = [int(pes[r][2]) for r in range(4)]
    for m in ma:
        r, dist = PR.infer_dir(L, anchor.rb, m.rb)
        if pes[r][0] <= dist <= pes[r][1]:
            skip[r] = 1
    if all(skip):
        return 0, 0
    l_ms = len(mate)
    n = added = 0
    for r in range(4):
        if skip[r]:
            continue
        win = window(anchor, r, pes[r], l_ms, L, contig_off, P)
        if win is not None:
            rb, re, is_rev = win
            seq = revcomp(mate) if is_rev else np.asarray(mate)
            score, te, qe, score2, _, qb, tb = sw(seq, text[rb:re], P)
            n += 1
            if score >= P["min_seed_len"] and qb >= 0:
                B = Reg()
                B.rid = anchor.rid
                B.qb, B.qe = (l_ms - (qe + 1), l_ms - qb) if is_rev else (qb, qe + 1)
                B.rb, B.re = (2 * L - (rb + te + 1), 2 * L - (rb + tb)) if is_rev else (rb + tb, rb + te + 1)
                B.score, B.csub, B.secondary, B.sel = score, score2, -1, -1
                B.seedcov = min(B.re - B.rb, B.qe - B.qb) >> 1
                B.win = (2 * L - re, re - rb) if is_rev else (rb, re - rb)
                at = next((i for i, x in enumerate(ma) if x.score < B.score), len(ma))
                ma.insert(at, B)
                added += 1
        if n > 0:
            for x in ma:
                x.excluded = False
            ma[:] = RG.dedup(ma, P)
    return n, added


# ---- rule 4: the regs stage's mapq and report rules with csub, and frac_rep = 0 for a region without a seed
def frac_rep_of(x, l_rep):
    return f32(0) if x.seedlen0 == 0 else f32(l_rep) / f32(x.lq)


def _ulps(x):
    return (x, math.nextafter(x, -math.inf), math.nextafter(x, math.inf))


def mapq_values(x, l_rep, P):
    """x.lq: the lq of the region's seed record (not read when seedlen0 == 0)."""
    sub = x.sub if x.sub else P["min_seed_len"] * P["a"]
    sub = max(sub, x.csub)
    if sub >= x.score:
        return [0]
    l = max(x.qe - x.qb, x.re - x.rb)
    if l < 1 or x.score == 0:
        return [0]
    identity = 1. - float(l * P["a"] - x.score) / float(P["a"] + P["b"]) / float(l)
    frac_rep = frac_rep_of(x, l_rep)
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


def mapq_se(x, l_rep, P):
    return mapq_values(x, l_rep, P)[0]


def report(a, l_rep, P):
    """-> (number reported, number of boundary inputs)."""
    boundary = 0
    for x in a:
        x.mapq = 0
        if x.secondary < 0:
            v = mapq_values(x, l_rep, P)
            boundary += len(set(v)) > 1
            x.mapq = v[0]
    k, first = 0, None
    for x in a:
        x.flag, x.sel = 0, -1
        if x.score < P["T"] or x.secondary >= 0:
            continue
        x.flag = 1
        if k > 0:
            x.flag |= 0x800
            x.mapq = min(x.mapq, first.mapq)
        else:
            first = x
        x.sel = k
        k += 1
    return k, boundary


def decision_cap(c, P):
    """The cap on q_se in the paired decision: raw(c.score - c.csub)."""
    return int(6.02 * float(c.score - c.csub) / float(P["a"]) + .499)


# ---- the insert-size estimate alone
def pestat(regs, reg_off, L, P):
    """-> (PESTAT_DTYPE[4], boundary count).  P: mem_pair_ref's parameters."""
    regs = np.asarray(regs).view(RG.REG_DTYPE)
    n_pairs = (len(reg_off) - 1) // 2
    ends = [tuple([PR.Reg(x) for x in regs[int(reg_off[2 * p + e]):int(reg_off[2 * p + e + 1])]] for e in (0, 1)) for p in range(n_pairs)]
    bd = PR.Boundary()
    pes = PR.pestat(PR.insert_sizes(ends, L, P), bd)
    out = np.zeros(4, dtype=PESTAT_DTYPE)
    for d, (lo, hi, failed, avg, std) in enumerate(pes):
        out[d] = (lo, hi, failed, 0, avg, std)
    return out, bd.n


def pes_tuples(pes):
    if isinstance(pes, np.ndarray) and pes.dtype == PESTAT_DTYPE:
        return [(int(x["low"]), int(x["high"]), int(x["failed"]), float(x["avg"]), float(x["std"])) for x in pes]
    return [tuple(x) for x in pes]


# ---- the stage
def rescue_all(regs, reg_off, seeds, l_rep, read_off, read_len, text, qer, L, contig_off, pes, P=None, pair_id0=0, seed_cap=None,
               xreg_cap=None, xseed_cap=None, xsel_cap=None):
    """Every pair -> dict(xregs REG_DTYPE, xreg_off, n_xregs, xseeds SEED_DTYPE[xseed_cap], n_xseeds, xsel_seeds SEED_DTYPE[xsel_cap],
    xsel_res int32[xsel_cap, 8], n_xsel, stats STAT_DTYPE[n_pairs], boundary).  seed_cap: where the new seed records begin (the
    number of seeds by default); the capacities default to what suffices."""
    P = P or params()
    regs = np.asarray(regs).view(REG_DTYPE)
    seeds = np.asarray(seeds, dtype=SEED_DTYPE)
    text, qer = np.asarray(text), np.asarray(qer)
    pes = pes_tuples(pes)
    n_pairs = (len(reg_off) - 1) // 2
    seed_cap = len(seeds) if seed_cap is None else seed_cap
    out, off, new_seeds, lst, stats, boundary = [], [0], [], [], [], 0
    for p in range(n_pairs):
        g = [int(reg_off[2 * p + e]) for e in (0, 1, 2)]
        given = [[Reg(x) for x in regs[g[e]:g[e + 1]]] for e in (0, 1)]
        for x in given[0] + given[1]:
            x.lq = int(seeds[x.seed]["lq"])
        a = [sorted(given[e], key=lambda x: (-x.score, x.rb, x.qb)) for e in (0, 1)]
        b = [[x for x in a[e] if x.score >= a[e][0].score - P["pen_unpaired"]][:P["max_matesw"]] for e in (0, 1)]     # ([] of an empty end)
        b = [[(x.rb, x.rid) for x in b[e]] for e in (0, 1)]         # fixed before any rescue
        seq = [qer[int(read_off[2 * p + e]):int(read_off[2 * p + e]) + int(read_len[2 * p + e])] for e in (0, 1)]
        n_sw = n_added = 0
        for e in (0, 1):
            for rb, rid in b[e]:
                anchor = Reg()
                anchor.rb, anchor.rid = rb, rid
                n, ad = matesw(anchor, seq[1 - e], a[1 - e], pes, L, contig_off, text, P)
                n_sw += n
                n_added += ad
        n_kept = 0
        for e in (0, 1):
            r = 2 * p + e
            if n_sw == 0:
                final = given[e]                     # byte-equal to the input
            else:
                final = RG.mark_primary(a[e], 2 * (pair_id0 + p) + e, P)
                _, bd = report(final, int(l_rep[r]), P)
                boundary += bd
            for x in final:
                if x.win is not None:
                    x.read = r
                    x.seed = seed_cap + len(new_seeds)
                    new_seeds.append((int(read_off[r]), x.win[0], int(read_len[r]), x.win[1], x.qb, x.rb - x.win[0], 0, 0))
                    x.roff = x.win[0]
                    n_kept += 1
                else:
                    x.roff = int(seeds[x.seed]["roff"])
                if x.flag & 1:
                    x.sel = len(lst)
                    lst.append(x)
                out.append(x.row())
            off.append(len(out))
        stats.append((n_sw, n_added, n_kept, 0))
    n_xseeds = seed_cap + len(new_seeds)
    xreg_cap = len(out) if xreg_cap is None else xreg_cap
    xseed_cap = n_xseeds if xseed_cap is None else xseed_cap
    xsel_cap = len(out) if xsel_cap is None else xsel_cap
    xseeds = np.zeros(xseed_cap, dtype=SEED_DTYPE)
    k = min(len(seeds), seed_cap, xseed_cap)
    xseeds[:k] = seeds[:k]
    for i, s in enumerate(new_seeds):
        if seed_cap + i < xseed_cap:
            xseeds[seed_cap + i] = s
    all_seeds = np.zeros(n_xseeds, dtype=SEED_DTYPE)
    all_seeds[:min(len(seeds), seed_cap)] = seeds[:seed_cap]
    if new_seeds:
        all_seeds[seed_cap:] = np.array(new_seeds, dtype=SEED_DTYPE)
    xsel_seeds = np.zeros(xsel_cap, dtype=SEED_DTYPE)
    xsel_res = np.full((xsel_cap, 8), -1, dtype=np.int32)
    for i, x in enumerate(lst[:xsel_cap]):
        xsel_seeds[i] = all_seeds[x.seed]
        xsel_res[i] = (x.score, x.truesc, x.qb, x.qe, x.rb - x.roff, x.re - x.roff, x.w, 0)
    xregs = np.array(out, dtype=REG_DTYPE).reshape(-1)
    return dict(xregs=xregs[:xreg_cap], xreg_off=np.array(off, dtype=np.int64), n_xregs=len(out), xseeds=xseeds, n_xseeds=n_xseeds,
                xsel_seeds=xsel_seeds, xsel_res=xsel_res, n_xsel=len(lst), stats=np.array(stats, dtype=STAT_DTYPE).reshape(-1),
                boundary=boundary)
