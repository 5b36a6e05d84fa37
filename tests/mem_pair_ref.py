"""Plain-Python restatement of the paired-end rules (include/gbx.h "paired-end"): bwa-mem's mem_pestat, mem_pair and
the decision part of mem_sam_pe without mate rescue, as the gbx_mem_pair_* entries are specified.  Serial, step by step; no device
code and nothing shared with genomicsbench_amd.mem_pair.

Boundary inputs: every quantity that is truncated by an `(int)` - qd of a candidate pair, the terms of q_pe, the terms of a
mapq, the bounds of the insert-size estimate - is noted when it lies within 1e-9 of an integer (far above what a few ulp in log,
erfc or sqrt can move it), and so is a candidate whose erfc is a nonzero subnormal; `pestat_bwa` forms S as bwa does, one value
at a time, and an estimate that differs from the agreed order's in low / high / failed, or in avg / std by more than 1e-12
relative, is noted too.  `boundary` in the result counts them; the tests require that their inputs hold none.
"""
import math

import numpy as np

from mem_regs_ref import REG_DTYPE, SEED_DTYPE, f32, hash_64

PESTAT_DTYPE = np.dtype([("low", "<i4"), ("high", "<i4"), ("failed", "<i4"), ("pad_", "<i4"), ("avg", "<f8"), ("std", "<f8")])
PAIR_DTYPE = np.dtype([("dist", "<i8"), ("score", "<i4"), ("sub", "<i4"), ("n_sub", "<i4"), ("n_cand", "<i4"), ("z0", "<i4"), ("z1", "<i4"),
                       ("q_pe", "<i4"), ("q_se0", "<i4"), ("q_se1", "<i4"), ("paired", "<i4"), ("proper", "<i4"), ("dir", "<i4")])
assert PESTAT_DTYPE.itemsize == 32 and PAIR_DTYPE.itemsize == 56
DEFAULTS = dict(a=1, b=4, o_del=6, e_del=1, o_ins=6, e_ins=1, min_seed_len=19, T=30, pen_unpaired=17, max_ins=10000, mapq_coef_len=50,
                mapq_coef_fac=float(np.float32(math.log(50.0))), mask_level=0.5, no_pairing=0)
M64 = (1 << 64) - 1
EPS = 1e-9


def params(**kw):
    p = dict(DEFAULTS)
    for k in kw:
        assert k in p, k
    p.update(kw)
    if "mapq_coef_len" in kw and "mapq_coef_fac" not in kw:
        p["mapq_coef_fac"] = float(np.float32(math.log(float(p["mapq_coef_len"]))))
    return p


class Boundary:
    """Counts the truncations that a last-bit difference could turn."""

    def __init__(self):
        self.n, self.what = 0, []

    def note(self, what):
        self.n += 1
        self.what.append(what)

    def trunc(self, x, what):
        """(int)x, towards zero."""
        if abs(x - round(x)) < EPS:
            self.note((what, x))
        return int(x)


def infer_dir(L, b1, b2):
    r1, r2 = b1 >= L, b2 >= L
    p2 = b2 if r1 == r2 else 2 * L - 1 - b2
    return (0 if r1 == r2 else 1) ^ (0 if p2 > b1 else 3), abs(p2 - b1)


class Reg:
    FIELDS = REG_DTYPE.names

    def __init__(self, row):
        for f in self.FIELDS:
            setattr(self, f, int(row[f]))

    def row(self):
        return tuple(getattr(self, f) for f in self.FIELDS)


# ---- 1: the insert-size estimate
def overlaps(x, t, P):
    b_max, e_min = max(x.qb, t.qb), min(x.qe, t.qe)
    if e_min <= b_max:
        return False
    min_l = min(x.qe - x.qb, t.qe - t.qb)
    return bool(f32(e_min - b_max) >= f32(min_l) * f32(P["mask_level"]))


def top_and_sub(a, P):
    """-> (the region first by (score desc, rb, qb), cal_sub)."""
    t = min(range(len(a)), key=lambda i: (-a[i].score, a[i].rb, a[i].qb))
    sub = [x.score for j, x in enumerate(a) if j != t and overlaps(x, a[t], P)]
    return a[t], (max(sub) if sub else P["min_seed_len"] * P["a"])


def insert_sizes(ends, L, P):
    """ends: per pair ([Reg of end 0], [Reg of end 1]) -> the four lists of insert sizes, in pair order."""
    vals = [[], [], [], []]
    for a0, a1 in ends:
        if not a0 or not a1:
            continue
        (t0, s0), (t1, s1) = top_and_sub(a0, P), top_and_sub(a1, P)
        if float(s0) > 0.8 * float(t0.score) or float(s1) > 0.8 * float(t1.score):
            continue
        if t0.rid != t1.rid:
            continue
        d, dist = infer_dir(L, t0.rb, t1.rb)
        if 1 <= dist <= P["max_ins"]:
            vals[d].append(dist)
    return vals


def pestat_one(vals, bd, bwa_order=False):
    """One direction -> (low, high, failed, avg, std).  bwa_order: S one value at a time, as bwa adds it."""
    n = len(vals)
    if n < 10:
        return (0, 0, 1, 0., 0.)
    q = sorted(vals)
    p25, p50, p75 = (q[int(k * float(n) + .499)] for k in (.25, .50, .75))
    low = max(bd.trunc(float(p25) - 2.0 * float(p75 - p25) + .499, "pestat low"), 1)
    high = bd.trunc(float(p75) + 2.0 * float(p75 - p25) + .499, "pestat high")
    inside = [v for v in q if low <= v <= high]
    x = len(inside)
    avg = float(sum(inside)) / float(x)
    S = 0.
    if bwa_order:
        for v in inside:
            S += (float(v) - avg) * (float(v) - avg)
    else:
        count = {}
        for v in inside:
            count[v] = count.get(v, 0) + 1
        for v in sorted(count):
            S += float(count[v]) * ((float(v) - avg) * (float(v) - avg))
    std = math.sqrt(S / float(x))
    low = bd.trunc(float(p25) - 3.0 * float(p75 - p25) + .499, "pestat low")
    high = bd.trunc(float(p75) + 3.0 * float(p75 - p25) + .499, "pestat high")
    if float(low) > avg - 4.0 * std:
        low = bd.trunc(avg - 4.0 * std + .499, "pestat low 4 std")
    if float(high) < avg + 4.0 * std:
        high = bd.trunc(avg + 4.0 * std + .499, "pestat high 4 std")
    return (max(low, 1), high, 0, avg, std)


def pestat_of(vals, bd, bwa_order=False):
    """The four lists -> four (low, high, failed, avg, std)."""
    pes = [pestat_one(v, bd, bwa_order) for v in vals]
    most = max(len(v) for v in vals)
    return [(lo, hi, 1, avg, std) if not failed and float(len(v)) < 0.05 * float(most) else (lo, hi, failed, avg, std)
            for (lo, hi, failed, avg, std), v in zip(pes, vals)]


def pestat(vals, bd):
    """The estimate in the agreed summation order; an estimate that bwa's order would change is a boundary input."""
    pes, bwa = pestat_of(vals, bd), pestat_of(vals, Boundary(), True)
    for d, (x, y) in enumerate(zip(pes, bwa)):
        if x[:3] != y[:3] or any(abs(u - v) > 1e-12 * abs(v) for u, v in zip(x[3:], y[3:])):
            bd.note(("pestat_bwa", d, x, y))
    return pes


def pestat_bwa(vals):
    return pestat_of(vals, Boundary(), True)


# ---- 2: pairing
def pair_q(si, sk, dist, pe, P, bd):
    """q of a candidate pair at insert `dist` under the direction's estimate."""
    avg, std = pe[3], pe[4]
    if std == 0.:                                    # (an estimate from one repeated value: the division has no IEEE answer here)
        ns = math.inf if float(dist) != avg else math.nan
    else:
        ns = (float(dist) - avg) / std
    if math.isnan(ns):
        return 0
    e = math.erfc(abs(ns) * math.sqrt(.5))
    if e == 0.:                                      # log(0) = -inf: tested before the cast
        return 0
    qd = float(si + sk) + .721 * math.log(2. * e) * float(P["a"]) + .499
    if qd > -EPS and e < 2.3e-308:
        bd.note(("subnormal erfc", dist))
    if qd <= 0.:
        if qd > -EPS:
            bd.note(("qd", qd))
        return 0
    return bd.trunc(qd, "qd")


def mem_pair(a0, a1, pes, L, contig_off, pair_id, P, bd):
    """-> (score, sub, n_sub, n_cand, z) with z None when there is no candidate."""
    keys = []
    for e, a in enumerate((a0, a1)):
        for i, x in enumerate(a):
            rev = x.rb >= L
            fwd = 2 * L - 1 - x.rb if rev else x.rb
            keys.append(((x.rid << 32 | ((fwd - int(contig_off[x.rid])) & M64)) & M64, x.score << 32 | i << 2 | int(rev) << 1 | e))
    keys.sort()
    last = [-1] * 4
    cand = []
    for i, (xi, yi) in enumerate(keys):
        for r in (0, 1):
            d = r << 1 | (yi >> 1 & 1)
            if pes[d][2]:
                continue
            which = r << 1 | ((yi & 1) ^ 1)
            for k in range(last[which], -1, -1):
                xk, yk = keys[k]
                if (yk & 3) != which:
                    continue
                dist = xi - xk
                if dist > pes[d][1]:
                    break
                if dist < pes[d][0]:
                    continue
                q = pair_q(yi >> 32, yk >> 32, dist, pes[d], P, bd)
                Y = k << 32 | i
                cand.append((q << 32 | (hash_64(Y ^ ((pair_id << 8) & M64)) & 0xffffffff), Y))
        last[yi & 3] = i
    if not cand:
        return 0, 0, 0, 0, None
    cand.sort()
    X, Y = cand[-1]
    z = [0, 0]
    for y in (keys[Y >> 32][1], keys[Y & 0xffffffff][1]):
        z[y & 1] = (y & 0xffffffff) >> 2
    sub = cand[-2][0] >> 32 if len(cand) > 1 else 0
    tmp = max(P["a"] + P["b"], P["o_del"] + P["e_del"], P["o_ins"] + P["e_ins"])
    n_sub = sum(1 for c in cand[:-1] if sub - (c[0] >> 32) <= tmp)
    return X >> 32, sub, n_sub, len(cand), z


# ---- 3: the decision
def mapq_se(c, l_rep, lq, P, bd):
    """DESIGN 3.12 rule 4 on the region's current sub and sub_n, without its secondary test."""
    a = P["a"]
    sub = c.sub if c.sub else P["min_seed_len"] * a
    if sub >= c.score:
        return 0
    l = max(c.qe - c.qb, c.re - c.rb)
    if l < 1 or c.score == 0:
        return 0
    identity = 1. - float(l * a - c.score) / float(a + P["b"]) / float(l)
    t = 1. if l < P["mapq_coef_len"] else float(f32(P["mapq_coef_fac"])) / math.log(float(l))
    t *= identity * identity
    mapq = bd.trunc(6.02 * float(c.score - sub) / float(a) * t * t + .499, "mapq")
    if c.sub_n > 0:
        mapq -= bd.trunc(4.343 * math.log(float(c.sub_n + 1)) + .499, "mapq sub_n")
    mapq = max(0, min(60, mapq))
    frac_rep = f32(l_rep) / f32(lq)
    return bd.trunc(float(mapq) * (1. - float(frac_rep)) + .499, "mapq frac_rep")


def raw_mapq(d, P, bd):
    return bd.trunc(6.02 * float(d) / float(P["a"]) + .499, "raw mapq")


def decide(a, l_rep, lq, pes, L, contig_off, pair_id, P, bd):
    """One pair.  a: ([Reg], [Reg]), changed in place as d_pregs is -> its PAIR_DTYPE row."""
    score = sub = n_sub = n_cand = 0
    z = None
    if a[0] and a[1] and not P["no_pairing"]:
        score, sub, n_sub, n_cand, z = mem_pair(a[0], a[1], pes, L, contig_off, pair_id, P, bd)
    multi = any(x.secondary < 0 and x.score >= P["T"] for e in (0, 1) for x in a[e][1:])
    q_pe, q_se, paired, proper = 0, [0, 0], 0, 0
    if score > 0 and not multi:
        paired = 1
        score_un = a[0][0].score + a[1][0].score - P["pen_unpaired"]
        subo = max(sub, score_un)
        q_pe = raw_mapq(score - subo, P, bd)
        if n_sub > 0:
            q_pe -= bd.trunc(4.343 * math.log(float(n_sub + 1)) + .499, "q_pe n_sub")
        q_pe = max(0, min(60, q_pe))
        frac = f32(l_rep[0]) / f32(lq[0]) + f32(l_rep[1]) / f32(lq[1])
        q_pe = bd.trunc(float(q_pe) * (1. - .5 * float(frac)) + .499, "q_pe frac_rep")
        if score > score_un:
            proper = 1
            for e in (0, 1):
                c = a[e][z[e]]
                if c.secondary >= 0:
                    c.sub, c.secondary = a[e][c.secondary].score, -2
                q = mapq_se(c, l_rep[e], lq[e], P, bd)
                q = q if q > q_pe else min(q_pe, q + 40)
                q_se[e] = min(q, raw_mapq(c.score, P, bd))
        else:
            z = [0, 0]
            q_se = [mapq_se(a[e][0], l_rep[e], lq[e], P, bd) for e in (0, 1)]
        for e in (0, 1):
            for i, x in enumerate(a[e]):
                x.flag, x.sel = (1, 0) if i == z[e] else (0, -1)
            a[e][z[e]].mapq = q_se[e]
    else:
        z = [0 if a[e] and a[e][0].score >= P["T"] else -1 for e in (0, 1)]
        q_se = [a[e][0].mapq if z[e] == 0 else 0 for e in (0, 1)]
        if not P["no_pairing"] and z == [0, 0] and a[0][0].rid == a[1][0].rid:
            d, dist = infer_dir(L, a[0][0].rb, a[1][0].rb)
            proper = int(not pes[d][2] and pes[d][0] <= dist <= pes[d][1])
        for e in (0, 1):                             # sel: the place among the read's reported regions
            k = 0
            for x in a[e]:
                x.sel = -1
                if x.flag & 1:
                    x.sel = k
                    k += 1
    d, dist = (-1, 0) if min(z) < 0 else infer_dir(L, a[0][z[0]].rb, a[1][z[1]].rb)
    return (dist, score, sub, n_sub, n_cand, z[0], z[1], q_pe, q_se[0], q_se[1], paired, proper, d)


def pair_all(regs, reg_off, sel_seeds, sel_res, seeds, l_rep, L, contig_off, P=None, pair_id0=0, pes_in=None, psel_cap=None):
    """Every pair -> dict(pes PESTAT_DTYPE[4], pairs PAIR_DTYPE, pregs REG_DTYPE, psel_seeds SEED_DTYPE[psel_cap], psel_res
    int32[psel_cap, 8], n_psel, boundary, notes, insert_sizes).  regs / reg_off: the regs stage's output for 2 n_pairs interleaved
    reads; sel_seeds / sel_res: its CIGAR list; pes_in: None or four (low, high, failed, avg, std).  psel_cap defaults to the
    number of regions, which always suffices."""
    P = P or params()
    regs = np.asarray(regs, dtype=REG_DTYPE)
    seeds = np.asarray(seeds, dtype=SEED_DTYPE)
    sel_seeds = np.asarray(sel_seeds, dtype=SEED_DTYPE)
    sel_res = np.ascontiguousarray(sel_res, dtype=np.int32).reshape(-1, 8)
    n_pairs = (len(reg_off) - 1) // 2
    assert len(reg_off) == 2 * n_pairs + 1
    psel_cap = len(regs) if psel_cap is None else psel_cap
    bd = Boundary()
    ends = [tuple([Reg(x) for x in regs[int(reg_off[2 * p + e]):int(reg_off[2 * p + e + 1])]] for e in (0, 1)) for p in range(n_pairs)]
    vals = None
    if pes_in is None:
        vals = insert_sizes(ends, L, P)
        pes = pestat(vals, bd)
    else:
        pes = [tuple(x) for x in pes_in]
    pairs, pregs, lst = [], [], []
    for p, a in enumerate(ends):
        lr = [int(l_rep[2 * p + e]) for e in (0, 1)]
        lq = [int(seeds[a[e][0].seed]["lq"]) if a[e] else 1 for e in (0, 1)]
        pairs.append(decide(a, lr, lq, pes, L, contig_off, pair_id0 + p, P, bd))
        for e in (0, 1):
            base = len(lst)
            for x in a[e]:
                if x.sel >= 0:
                    lst.append((x, int(regs[len(pregs)]["sel"])))
                    x.sel += base
                pregs.append(x.row())
    psel_seeds = np.zeros(psel_cap, dtype=SEED_DTYPE)
    psel_res = np.full((psel_cap, 8), -1, dtype=np.int32)
    for k, (x, old) in enumerate(lst[:psel_cap]):
        if 0 <= old < len(sel_seeds):                # a copy of the regs stage's records
            psel_seeds[k], psel_res[k] = sel_seeds[old], sel_res[old]
        else:                                        # built as 3.12 rule 5 builds them
            s = seeds[x.seed]
            psel_seeds[k] = s
            psel_res[k] = (x.score, x.truesc, x.qb, x.qe, x.rb - int(s["roff"]), x.re - int(s["roff"]), x.w, 0)
    out_pes = np.zeros(4, dtype=PESTAT_DTYPE)
    for d, (lo, hi, failed, avg, std) in enumerate(pes):
        out_pes[d] = (lo, hi, failed, 0, avg, std)
    return dict(pes=out_pes, pairs=np.array(pairs, dtype=PAIR_DTYPE).reshape(-1), pregs=np.array(pregs, dtype=REG_DTYPE).reshape(-1),
                psel_seeds=psel_seeds, psel_res=psel_res, n_psel=len(lst), boundary=bd.n, notes=bd.what, insert_sizes=vals)
