"""Sequential restatement of minimap2 behind the chain scores: chain ends and backtrack (the second half of
mm_chain_dp), chain order, mm_gen_regs, mm_set_parent, mm_select_sub, mm_set_mapq and the PAF line.  Plain Python integers and
np.float32, one step at a time in the order minimap2 takes them; this file pins the device code (minimap2's source is not part of
the reference tree).  Where minimap2 leaves an order to an unstable sort, the rule here fixes it (the keys carry what breaks a tie)."""
import math

import numpy as np

from mm_ref import hash64

M64 = (1 << 64) - 1
M32 = 0xffffffff
F = np.float32
DEFAULTS = dict(min_cnt=3, min_chain_score=40, mask_level=0.5, pri_ratio=0.8, best_n=5, min_diff=30)
REG_FIELDS = ("id", "parent", "score", "subsc", "cnt", "as", "rid", "rev", "rs", "re", "qs", "qe", "mlen", "blen", "n_sub", "mapq", "hash", "read")


def i32(v):
    v &= M32
    return v - (1 << 32) if v >> 31 else v


def par(p, i):
    """chain leaves p[i] < i; anything else counts as none"""
    j = int(p[i])
    return j if 0 <= j < i else -1


def chains(f, p, v, ax, ay, min_sc, min_cnt, stats=None):
    """Steps 1-3 -> (u [score << 32 | c], chained anchors [(x, y)]) in step-3 order.  stats: a dict whose counters of the paths
    taken are raised (the case generators assert their coverage with it)."""
    st = stats if stats is not None else {}
    bump = lambda k: st.__setitem__(k, st.get(k, 0) + 1)
    n = len(f)
    t = [0] * n
    for j in range(n):
        if par(p, j) >= 0:
            t[par(p, j)] = 1
    keys = []
    for i in range(n):
        if t[i] == 0 and v[i] >= min_sc:
            j = i
            while j >= 0 and f[j] < v[j]:
                j = par(p, j)
            if j < 0:
                j = i
                bump("off_root")
            keys.append((int(f[j]) & M32) << 32 | j)
    keys.sort(reverse=True)
    if not keys:
        bump("no_end")
    t = [0] * n
    out = []                                                  # (score, anchors ascending)
    cut = set()                                               # anchors marked by chains that min_cnt dropped
    for rank, u in enumerate(keys):
        j, s = u & M32, i32(u >> 32)
        if t[j]:
            bump("dup_peak" if rank and keys[rank - 1] == u else "peak_in_walk")
        taken = []
        while True:
            taken.append(j)
            t[j] = 1
            j = par(p, j)
            if not (j >= 0 and t[j] == 0):
                break
        c = len(taken)
        if j < 0:
            keep, sc = c >= min_cnt, s
        else:
            sc = s - int(f[j])
            keep = sc >= min_sc and c >= min_cnt
            bump("stop_kept" if keep else "stop_dropped")
            if j in cut:
                bump("cut_by_dropped")
        if not keep and c < min_cnt and (j < 0 or sc >= min_sc):
            cut.update(taken)
        if keep:
            out.append((sc, taken[::-1]))
    order = sorted(range(len(out)), key=lambda i: (int(ax[out[i][1][0]]), i))
    u = [(out[i][0] & M32) << 32 | len(out[i][1]) for i in order]
    a = [(int(ax[j]), int(ay[j])) for i in order for j in out[i][1]]
    return u, a


def gen_regs(u, a, qlen, hash_):
    """Step 4 -> list of region dicts in order"""
    z = []
    k = 0
    for ui in u:
        c = ui & M32
        h = hash64((hash64(a[k][0], M64) + hash64(a[k][1], M64)) & M64 ^ hash_, M64) & M32
        z.append((ui ^ h, k << 32 | c))
        k += c
    z.sort(reverse=True)
    regs = []
    for i, (zx, zy) in enumerate(z):
        g = dict(id=i, parent=-1, score=i32(zx >> 32), hash=zx & M32, cnt=zy & M32, subsc=0, n_sub=0, mapq=0)
        g["as"] = zy >> 32
        first, last = a[g["as"]], a[g["as"] + g["cnt"] - 1]
        sp = first[1] >> 32 & 0xff
        g["rev"], g["rid"] = first[0] >> 63, (first[0] << 1 & M64) >> 33
        g["rs"], g["re"] = max(i32(first[0]) + 1 - sp, 0), i32(last[0]) + 1
        q0, q1 = i32(first[1]) + 1 - sp, i32(last[1]) + 1
        g["qs"], g["qe"] = (qlen - q1, qlen - q0) if g["rev"] else (q0, q1)
        mlen = blen = sp
        for m in range(g["as"] + 1, g["as"] + g["cnt"]):
            tl, ql, span = i32(a[m][0]) - i32(a[m - 1][0]), i32(a[m][1]) - i32(a[m - 1][1]), a[m][1] >> 32 & 0xff
            blen += max(tl, ql)
            mlen += span if tl > span and ql > span else min(tl, ql)
        g["mlen"], g["blen"] = mlen, blen
        regs.append(g)
    return regs


def set_parent(regs, mask_level):
    """Step 5, in place"""
    if not regs:
        return
    mask_level = F(mask_level)
    regs[0]["parent"] = 0
    w = [0]
    for i in range(1, len(regs)):
        ri = regs[i]
        si, ei = ri["qs"], ri["qe"]
        cov = []
        for j in w:
            sj, ej = regs[j]["qs"], regs[j]["qe"]
            if ej <= si or sj >= ei:
                continue
            cov.append((max(sj, si), min(ej, ei)))
        uncov = 0
        if cov:
            x = si
            for cs, ce in sorted(cov):
                if cs > x:
                    uncov += cs - x
                x = max(x, ce)
            if ei > x:
                uncov += ei - x
        taken = False
        for j in w:
            rp = regs[j]
            sj, ej = rp["qs"], rp["qe"]
            if ej <= si or sj >= ei:
                continue
            mn, mx = min(ej - sj, ei - si), max(ej - sj, ei - si)
            ol = min(ei, ej) - max(si, sj)
            if F(ol) / F(mn) - F(uncov) / F(mx) > mask_level:
                ri["parent"] = j
                rp["subsc"] = max(rp["subsc"], ri["score"])
                if ri["cnt"] >= rp["cnt"]:
                    rp["n_sub"] += 1
                taken = True
                break
        if not taken:
            w.append(i)
            ri["parent"], ri["n_sub"] = i, 0


def select_sub(regs, pri_ratio, min_diff, best_n):
    """Step 6 -> the kept regions, renumbered"""
    if not F(pri_ratio) > 0:
        return regs
    kept, n2 = [], 0
    for i, g in enumerate(regs):
        if g["parent"] == i:
            kept.append(g)
            continue
        rp = regs[g["parent"]]
        if (F(g["score"]) >= F(rp["score"]) * F(pri_ratio) or g["score"] + min_diff >= rp["score"]) and n2 < best_n:
            if not all(g[k] == rp[k] for k in ("qs", "qe", "rid", "rs", "re")):
                kept.append(g)
                n2 += 1
    new = {g["id"]: k for k, g in enumerate(kept)}
    for g in kept:
        g["id"], g["parent"] = new[g["id"]], new[g["parent"]]
    return kept


def L(n):
    return F(math.log(float(n)))


def set_mapq(regs, rep_len, min_chain_score):
    """Step 7, in place; float32, every operation rounded on its own"""
    sum_sc = sum(g["score"] for g in regs if g["parent"] == g["id"])
    with np.errstate(all="ignore"):
        uniq_ratio = F(sum_sc) / F(sum_sc + rep_len)
        for g in regs:
            if g["parent"] != g["id"]:
                g["mapq"] = 0
                continue
            pen_s1 = (F(1.0) if g["score"] > 100 else F(0.01) * F(g["score"])) * uniq_ratio
            pen_cm = min(pen_s1, F(1.0) if g["cnt"] > 10 else F(0.1) * F(g["cnt"]))
            sub = max(g["subsc"], min_chain_score)
            x = F(sub) / F(g["score"])
            q = int(pen_cm * F(40.0) * (F(1.0) - x) * L(g["score"]))
            q -= int(F(4.343) * L(g["n_sub"] + 1) + F(.499))
            g["mapq"] = min(max(q, 0), 60)


def map_read(f, p, v, ax, ay, qlen, rep_len, hash_, read=0, **kw):
    """Steps 1-7 of one read -> (u, chained anchors, regions)"""
    stats = kw.pop("stats", None)
    P = dict(DEFAULTS, **kw)
    u, a = chains(f, p, v, ax, ay, P["min_chain_score"], P["min_cnt"], stats)
    regs = gen_regs(u, a, qlen, hash_)
    set_parent(regs, P["mask_level"])
    regs = select_sub(regs, P["pri_ratio"], P["min_diff"], P["best_n"])
    set_mapq(regs, rep_len, P["min_chain_score"])
    for g in regs:
        g["read"] = read
    return u, a, regs


def map_batch(off, ax, ay, f, p, v, qlen, rep_len, hashes, **kw):
    """-> dict of the flat arrays a device call leaves: chain_off, u, cax / cay (a read's chained anchors at off[r]), n_chained,
    reg_off, regs (a dict of int64 arrays by field)"""
    n = len(off) - 1
    chain_off, reg_off = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    us, regs = [], []
    cax, cay = np.zeros(len(ax), np.uint64), np.zeros(len(ax), np.uint64)
    n_chained = np.zeros(n, np.int32)
    for r in range(n):
        lo, hi = int(off[r]), int(off[r + 1])
        u, a, g = map_read(f[lo:hi], p[lo:hi], v[lo:hi], ax[lo:hi], ay[lo:hi], int(qlen[r]), int(rep_len[r]), int(hashes[r]), r, **kw)
        us += u
        regs += g
        for i, (x, y) in enumerate(a):
            cax[lo + i], cay[lo + i] = x, y
        n_chained[r] = len(a)
        chain_off[r + 1], reg_off[r + 1] = len(us), len(regs)
    return dict(chain_off=chain_off, u=np.array(us, dtype=np.uint64), cax=cax, cay=cay, n_chained=n_chained, reg_off=reg_off,
                regs={k: np.array([g[k] for g in regs], dtype=np.int64) for k in REG_FIELDS})


def x31(name):
    if isinstance(name, str):
        name = name.encode()
    if not name:
        return 0
    h = name[0]
    for c in name[1:]:
        h = ((h << 5) - h + c) & M32
    return h


def wang(key):
    key = (key + (~(key << 15) & M32)) & M32
    key ^= key >> 10
    key = (key + (key << 3)) & M32
    key ^= key >> 6
    key = (key + (~(key << 11) & M32)) & M32
    key ^= key >> 16
    return key


def read_hash(name, qlen):
    return x31(name) ^ ((wang(qlen & M32) + wang(11)) & M32)


def paf_line(g, qname, qlen, tname, tlen, rep_len):
    pri = g["parent"] == g["id"]
    cols = [qname, qlen, g["qs"], g["qe"], "-" if g["rev"] else "+", tname, tlen, g["rs"], g["re"], g["mlen"], g["blen"], g["mapq"],
            "tp:A:P" if pri else "tp:A:S", "cm:i:%d" % g["cnt"], "s1:i:%d" % g["score"]]
    if pri:
        cols.append("s2:i:%d" % g["subsc"])
    cols.append("rl:i:%d" % rep_len)
    return "\t".join(str(c) for c in cols) + "\n"


def paf(regs, reg_off, qnames, qlens, tnames, tlens, rep_len):
    """regs: the dict of arrays of map_batch -> the text"""
    out = []
    for r in range(len(reg_off) - 1):
        for i in range(int(reg_off[r]), int(reg_off[r + 1])):
            g = {k: int(regs[k][i]) for k in REG_FIELDS}
            out.append(paf_line(g, qnames[r], int(qlens[r]), tnames[g["rid"]], int(tlens[g["rid"]]), int(rep_len[r])))
    return "".join(out)
