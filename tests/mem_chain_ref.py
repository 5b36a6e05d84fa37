"""Plain-Python restatement of the seed-chaining rules (include/gbx.h "seed chaining"): bwa-mem's mem_chain with
bns_intv2rid, mem_chain_flt and the window of mem_chain2aln, as the gbx_mem_chain_* entries are specified.  No device code and
nothing shared with genomicsbench_amd.mem_chain.  The chain heads are a sorted list searched with bisect; `lookup="scan"`
finds `lower` by a linear scan over all chains instead, so a slip in the tie rule of one cannot hide in the other.
"""
import bisect

import numpy as np

CHAIN_DTYPE = np.dtype([("pos", "<i8"), ("seed_off", "<i8"), ("rmax0", "<i8"), ("rmax1", "<i8"), ("read", "<i4"),
                        ("contig", "<i4"), ("n_seeds", "<i4"), ("weight", "<i4"), ("kept", "<i4"), ("pad_", "<i4")])
SEED_DTYPE = np.dtype([("qoff", "<i8"), ("roff", "<i8"), ("lq", "<i4"), ("rlen", "<i4"), ("qbeg", "<i4"), ("rbeg", "<i4"),
                       ("len", "<i4"), ("pad_", "<i4")])
DEFAULTS = dict(w=100, max_chain_gap=10000, max_occ=500, min_seed_len=19, min_chain_weight=0, max_chain_extend=1 << 30,
                mask_level=0.5, drop_ratio=0.5, a=1, o_del=6, e_del=1, o_ins=6, e_ins=1)


def params(**kw):
    p = dict(DEFAULTS)
    for k in kw:
        assert k in p, k
    p.update(kw)
    return p


def contig_of(rb, re, L, contig_off):
    """bns_intv2rid of [rb, re): the contig, or -1 when the interval crosses L or a contig boundary."""
    if rb < L < re:
        return -1
    b, e = (rb, re) if re <= L else (2 * L - re, 2 * L - rb)
    c = bisect.bisect_right(contig_off, b) - 1
    if c < 0 or c >= len(contig_off) - 1:
        return -1
    return c if e <= contig_off[c + 1] else -1


class Chain:
    def __init__(self, cid, contig, seed):
        self.cid, self.contig, self.seeds = cid, contig, [seed]
        self.pos = seed[2]
        self.first, self.kept, self.w = -1, 0, 0

    def beg(self):
        return self.seeds[0][0]

    def end(self):
        return self.seeds[-1][0] + self.seeds[-1][1]


def merge(C, p, c, L, P):
    """1: the seed (qbeg, len, rbeg) went into chain C or was dropped as contained; 0: it starts a new chain."""
    first, last = C.seeds[0], C.seeds[-1]
    if c != C.contig:
        return 0
    if p[0] >= first[0] and p[0] + p[1] <= last[0] + last[1] and p[2] >= first[2] and p[2] + p[1] <= last[2] + last[1]:
        return 1
    if (last[2] < L or first[2] < L) and p[2] >= L:
        return 0
    x, y = p[0] - last[0], p[2] - last[2]
    if y >= 0 and x - y <= P["w"] and y - x <= P["w"] and x - last[1] < P["max_chain_gap"] and y - last[1] < P["max_chain_gap"]:
        C.seeds.append(p)
        return 1
    return 0


def weight(C):
    def cover(k):
        end = w = 0
        for s in C.seeds:
            if s[k] >= end:
                w += s[1]
            elif s[k] + s[1] > end:
                w += s[k] + s[1] - end
            end = max(end, s[k] + s[1])
        return w
    return min(min(cover(0), cover(2)), (1 << 30) - 1)


def chain_filter(chains, P):
    """mem_chain_flt on the chains in chaining order -> the kept ones in the sorted order."""
    f32 = np.float32
    a = [C for C in chains if C.w >= P["min_chain_weight"]]
    a.sort(key=lambda C: -C.w)                    # stable: ties stay in chaining order
    for C in a:
        C.first, C.kept = -1, 0
    if not a:
        return []
    a[0].kept = 3
    K = [0]
    for i in range(1, len(a)):
        large, stopped = 0, False
        for j in K:
            b_max, e_min = max(a[j].beg(), a[i].beg()), min(a[j].end(), a[i].end())
            if e_min > b_max:
                min_l = min(a[i].end() - a[i].beg(), a[j].end() - a[j].beg())
                if f32(e_min - b_max) >= f32(min_l) * f32(P["mask_level"]) and min_l < P["max_chain_gap"]:
                    large = 1
                    if a[j].first < 0:
                        a[j].first = i
                    if f32(a[i].w) < f32(a[j].w) * f32(P["drop_ratio"]) and a[j].w - a[i].w >= 2 * P["min_seed_len"]:
                        stopped = True
                        break
        if not stopped:
            K.append(i)
            a[i].kept = 2 if large else 3
    for j in K:
        if a[j].first >= 0:
            a[a[j].first].kept = 1
    k, stop = 0, None
    for i, C in enumerate(a):
        if C.kept in (1, 2):
            k += 1
            if k >= P["max_chain_extend"]:
                stop = i
                break
    if stop is not None:
        for C in a[stop + 1:]:
            if C.kept < 3:
                C.kept = 0
    return [C for C in a if C.kept > 0]


def gap(q, P):
    gd = int((q * P["a"] - P["o_del"]) / P["e_del"] + 1.)
    gi = int((q * P["a"] - P["o_ins"]) / P["e_ins"] + 1.)
    return min(max(max(gd, gi), 1), 2 * P["w"])


def window(C, lq, L, contig_off, P):
    r0 = min(s[2] - (s[0] + gap(s[0], P)) for s in C.seeds)
    r1 = max(s[2] + s[1] + (lq - s[0] - s[1]) + gap(lq - s[0] - s[1], P) for s in C.seeds)
    r0, r1 = min(max(r0, 0), 2 * L), min(max(r1, 0), 2 * L)
    fwd = C.seeds[0][2] < L
    if r0 < L < r1:
        if fwd:
            r1 = L
        else:
            r0 = L
    c0, c1 = contig_off[C.contig], contig_off[C.contig + 1]
    lo, hi = (c0, c1) if fwd else (2 * L - c1, 2 * L - c0)
    return max(r0, lo), min(r1, hi)


def chain_read(seeds, L, contig_off, P, lookup="bisect"):
    """The chains of one read in chaining order (increasing pos, equal pos in creation order), and each seed's fate:
    a chain's creation id, "contained" or "skipped"."""
    heads, by_pos, made, fate = [], [], [], []           # heads: sorted pos; by_pos: the chains in that order
    for p in seeds:
        if p[2] < 0:
            fate.append("skipped")
            continue
        c = contig_of(p[2], p[2] + p[1], L, contig_off)
        if c < 0:
            fate.append("skipped")
            continue
        if lookup == "bisect":
            at = bisect.bisect_right(heads, p[2])
            lower = by_pos[at - 1] if at else None
        else:
            lower = None
            for C in made:                               # creation order: a later chain wins an equal pos
                if C.pos <= p[2] and (lower is None or C.pos >= lower.pos):
                    lower = C
            at = sum(1 for C in made if C.pos <= p[2])
        if lower is not None:
            n = len(lower.seeds)
            if merge(lower, p, c, L, P):
                fate.append(lower.cid if len(lower.seeds) > n else "contained")
                continue
        C = Chain(len(made), c, p)
        made.append(C)
        heads.insert(at, p[2])
        by_pos.insert(at, C)
        fate.append(C.cid)
    return by_pos, fate


def l_rep_of(smems, max_occ):
    b = e = l_rep = 0
    for m, n, s in smems:
        if s > max_occ:
            sb, se = m, n + 1
            if sb > e:
                l_rep += e - b
                b, e = sb, se
            else:
                e = max(e, se)
    return l_rep + e - b


def chain_all(m, n, s, smem_off, pos, pos_off, read_off, read_len, L, contig_off, P=None, lookup="bisect"):
    """Every read -> dict(chains CHAIN_DTYPE, chain_off, seeds SEED_DTYPE, l_rep, made: chains created per read,
    fates: per read the fate of every hit)."""
    P = P or params()
    contig_off = [int(x) for x in contig_off]
    pos = [int(x) for x in pos]
    chains, seeds, chain_off, l_rep, made, fates = [], [], [0], [], [], []
    for r in range(len(read_len)):
        j0, j1 = int(smem_off[r]), int(smem_off[r + 1])
        lq = int(read_len[r])
        rs = []
        for j in range(j0, j1):
            for h in range(int(pos_off[j]), int(pos_off[j + 1])):
                rs.append((int(m[j]), int(n[j]) + 1 - int(m[j]), pos[h]))
        l_rep.append(l_rep_of([(int(m[j]), int(n[j]), int(s[j])) for j in range(j0, j1)], P["max_occ"]))
        by_pos, fate = chain_read(rs, L, contig_off, P, lookup)
        made.append(len(by_pos))
        fates.append(fate)
        for C in by_pos:
            C.w = weight(C)
        for C in chain_filter(by_pos, P):
            r0, r1 = window(C, lq, L, contig_off, P)
            chains.append((C.pos, len(seeds), r0, r1, r, C.contig, len(C.seeds), C.w, C.kept, 0))
            for q, ln, rb in C.seeds:
                seeds.append((int(read_off[r]), r0, lq, r1 - r0, q, rb - r0, ln, 0))
        chain_off.append(len(chains))
    return dict(chains=np.array(chains, dtype=CHAIN_DTYPE), chain_off=np.array(chain_off, dtype=np.int64),
                seeds=np.array(seeds, dtype=SEED_DTYPE), l_rep=np.array(l_rep, dtype=np.int32), made=made, fates=fates)


def from_seeds(reads, lq=100):
    """Hand-built input: reads = [[(qbeg, len, rbeg), ...], ...] -> one single-hit SMEM per seed, reads laid out end to end.
    -> dict of the arrays chain_all and the entries take (s = 1 everywhere)."""
    lqs = [lq] * len(reads) if np.isscalar(lq) else list(lq)
    m, n, off, pos = [], [], [0], []
    for rs in reads:
        for q, ln, rb in rs:
            m.append(q)
            n.append(q + ln - 1)
            pos.append(rb)
        off.append(len(m))
    k = len(m)
    return dict(m=np.array(m, dtype=np.int64), n=np.array(n, dtype=np.int64), s=np.ones(k, dtype=np.int64),
                smem_off=np.array(off, dtype=np.int64), pos=np.array(pos, dtype=np.int64), pos_off=np.arange(k + 1, dtype=np.int64),
                read_off=np.concatenate([[0], np.cumsum(lqs)[:-1]]).astype(np.int64) if lqs else np.zeros(0, np.int64),
                read_len=np.array(lqs, dtype=np.int32))
