"""The rules of gbx_mem_cigar_* in plain Python: bwa-mem's mem_reg2aln / bwa_gen_cigar2 / ksw_global2 as the
issue states them.  UPSTREAM-KNOWLEDGE: bwa's source is not in the reference tree, so this restatement is the pin.

Two independent forms of the global alignment:
  global_rolling   ksw_global2's own shape: rolling H / E arrays, band offsets in the direction rows
  global_full      full (|T| + 1) x (|Q| + 1) matrices, cells outside the band INF, directions per cell, no offsets
and a C twin of the rolling form (tests/mem_cigar_ref.c, built on first use) for the inputs Python is too slow for.
All arithmetic stays far inside int32 for the lengths and costs tested, so Python's integers give the same values.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

INF = -0x40000000
SEED_DTYPE = np.dtype([("qoff", "<i8"), ("roff", "<i8"), ("lq", "<i4"), ("rlen", "<i4"), ("qbeg", "<i4"),
                       ("rbeg", "<i4"), ("len", "<i4"), ("pad_", "<i4")])
RESULT_DTYPE = np.dtype([("score", "<i4"), ("truesc", "<i4"), ("qb", "<i4"), ("qe", "<i4"), ("rb", "<i4"), ("re", "<i4"),
                         ("w", "<i4"), ("sc0", "<i4")])
ALN_DTYPE = np.dtype([("pos", "<i8"), ("cigar_off", "<i8"), ("rid", "<i4"), ("is_rev", "<i4"), ("n_cigar", "<i4"), ("nm", "<i4"),
                      ("score", "<i4"), ("w", "<i4"), ("tries", "<i4"), ("pad_", "<i4")])
M, I, D, S = 0, 1, 2, 4


def scmat(a=1, b=4):
    return [-1 if t == 4 or q == 4 else a if t == q else -b for t in range(5) for q in range(5)]


DEFAULTS = dict(mat=scmat(), o_del=6, e_del=1, o_ins=6, e_ins=1, w=100)


def params(**kw):
    p = dict(DEFAULTS)
    a, b = kw.pop("a", None), kw.pop("b", None)
    if a is not None or b is not None:
        p["mat"] = scmat(1 if a is None else a, 4 if b is None else b)
    for k, v in kw.items():
        assert k in p, k
        p[k] = list(v) if k == "mat" else v
    return p


def c_int(x):
    """(int) of a double: towards zero."""
    return int(x)


def infer_bw(l1, l2, score, a, q, e):
    if l1 == l2 and l1 * a - score < (q + e - a) << 1:
        return 0
    v = c_int(float(min(l1, l2) * a - score - q) / e + 2.)
    return max(v, abs(l1 - l2))


def first_band(p, lQ, lT, truesc, rw):
    a = p["mat"][0]
    w2 = max(infer_bw(lQ, lT, truesc, a, p["o_del"], p["e_del"]), infer_bw(lQ, lT, truesc, a, p["o_ins"], p["e_ins"]))
    if w2 > p["w"]:
        w2 = min(w2, rw)
    return w2


def band(p, lQ, lT, w_):
    a = p["mat"][0]
    max_ins = c_int(float(((lQ + 1) >> 1) * a - p["o_ins"]) / p["e_ins"] + 1.)
    max_del = c_int(float(((lQ + 1) >> 1) * a - p["o_del"]) / p["e_del"] + 1.)
    g = max(max_ins, max_del, 1)
    d = abs(lT - lQ)
    wb = (g + d + 1) >> 1
    wb = min(wb, w_)
    return max(wb, d + 3)


def _push(ops, op, n):
    if ops and ops[-1][0] == op:
        ops[-1][1] += n
    else:
        ops.append([op, n])


def global_rolling(Q, T, w, p, events=None):
    """ksw_global2 -> (score, [[op, len], ...] in sequence order).  events: a set that collects which ties occurred."""
    mat, o_del, e_del, o_ins, e_ins = p["mat"], p["o_del"], p["e_del"], p["o_ins"], p["e_ins"]
    oe_del, oe_ins = o_del + e_del, o_ins + e_ins
    lQ, lT = len(Q), len(T)
    n_col = min(lQ, 2 * w + 1)
    H, E = [INF] * (lQ + 1), [INF] * (lQ + 1)
    H[0] = 0
    for j in range(1, min(lQ, w) + 1):
        H[j] = -(o_ins + e_ins * j)
    z = []
    for i in range(lT):
        beg, end = max(i - w, 0), min(i + w + 1, lQ)
        h1 = -(o_del + e_del * (i + 1)) if beg == 0 else INF
        f = INF
        row = [0] * n_col
        for j in range(beg, end):
            m = H[j] + mat[T[i] * 5 + Q[j]]
            e = E[j]
            H[j] = h1
            if events is not None:
                if m == e and m > INF // 2:
                    events.add("m==e")
                if max(m, e) == f and f > INF // 2:
                    events.add("h==f")
            d = 0 if m >= e else 1
            h = max(m, e)
            d = d if h >= f else 2
            h = max(h, f)
            h1 = h
            t = m - oe_del
            e -= e_del
            if events is not None and e == t and e > INF // 2:
                events.add("e==t")
            d |= 1 << 2 if e > t else 0
            E[j] = max(e, t)
            t = m - oe_ins
            f -= e_ins
            if events is not None and f == t and f > INF // 2:
                events.add("f==t")
            d |= 2 << 4 if f > t else 0
            f = max(f, t)
            row[j - beg] = d
        H[end] = h1
        E[end] = INF
        z.append(row)
    score = H[lQ]
    i, k, which, ops = lT - 1, min(lT - 1 + w + 1, lQ) - 1, 0, []
    steps = 0
    while i >= 0 and k >= 0:
        which = (z[i][k - max(i - w, 0)] >> (which << 1)) & 3
        if which == 0:
            _push(ops, M, 1); i -= 1; k -= 1
        elif which == 1:
            _push(ops, D, 1); i -= 1
        else:
            _push(ops, I, 1); k -= 1
        steps += 1
        assert steps <= lQ + lT
    if i >= 0:
        _push(ops, D, i + 1)
    if k >= 0:
        _push(ops, I, k + 1)
    ops.reverse()
    return score, ops


def global_full(Q, T, w, p):
    """The same alignment from full matrices: Hm[r][c] = best score of T[:r] against Q[:c], cells outside the band INF; the
    three direction fields are kept per cell (r, c) in tables of their own and looked up by coordinates."""
    mat, o_del, e_del, o_ins, e_ins = p["mat"], p["o_del"], p["e_del"], p["o_ins"], p["e_ins"]
    lQ, lT = len(Q), len(T)
    inb = lambda r, c: 1 <= r <= lT and 1 <= c <= lQ and abs((r - 1) - (c - 1)) <= w
    Hm = [[INF] * (lQ + 1) for _ in range(lT + 1)]
    Em = [[INF] * (lQ + 2) for _ in range(lT + 2)]              # Em[r][c]: the deletion state arriving at cell (r, c)
    Fm = [[INF] * (lQ + 2) for _ in range(lT + 2)]              # Fm[r][c]: the insertion state arriving at cell (r, c)
    src = [[0] * (lQ + 1) for _ in range(lT + 1)]               # where H came from: 0 diagonal, 1 E, 2 F
    e_ext = [[0] * (lQ + 1) for _ in range(lT + 1)]             # the E leaving (r, c) downwards extends (1) or opens (0)
    f_ext = [[0] * (lQ + 1) for _ in range(lT + 1)]             # the F leaving (r, c) rightwards extends (2) or opens (0)
    Hm[0][0] = 0
    for c in range(1, min(lQ, w) + 1):
        Hm[0][c] = -(o_ins + e_ins * c)
    for r in range(1, lT + 1):
        if r - 1 - w <= 0:
            Hm[r][0] = -(o_del + e_del * r)
    for r in range(1, lT + 1):
        for c in range(1, lQ + 1):
            if not inb(r, c):
                continue
            m = Hm[r - 1][c - 1] + mat[T[r - 1] * 5 + Q[c - 1]]
            e = Em[r][c] if inb(r - 1, c) else INF
            f = Fm[r][c] if inb(r, c - 1) else INF
            h, s = m, 0
            if e > h:
                h, s = e, 1
            if f > h:
                h, s = f, 2
            Hm[r][c], src[r][c] = h, s
            opened = m - (o_del + e_del)
            e_ext[r][c] = 1 if e - e_del > opened else 0
            Em[r + 1][c] = max(e - e_del, opened)
            opened = m - (o_ins + e_ins)
            f_ext[r][c] = 2 if f - e_ins > opened else 0
            Fm[r][c + 1] = max(f - e_ins, opened)
    score = Hm[lT][lQ]
    r, c, state, rev = lT, min(lT - 1 + w + 1, lQ), 0, []
    while r >= 1 and c >= 1:
        state = src[r][c] if state == 0 else e_ext[r][c] if state == 1 else f_ext[r][c]
        if state == 0:
            rev.append(M); r -= 1; c -= 1
        elif state == 1:
            rev.append(D); r -= 1
        else:
            rev.append(I); c -= 1
    rev += [D] * r
    rev += [I] * c
    ops = []
    for op in reversed(rev):
        _push(ops, op, 1)
    return score, ops


def gen(p, Q, T, w_, lookup=global_rolling):
    if len(Q) == len(T) and w_ == 0:
        return sum(p["mat"][t * 5 + q] for q, t in zip(Q, T)), [[M, len(Q)]], None
    wb = band(p, len(Q), len(T), w_)
    score, ops = lookup(Q, T, wb, p)
    return score, ops, wb


def count_nm(ops, Q, T):
    """mismatching M positions + inserted bases + the deleted bases of every D that is neither first nor last."""
    nm, x, y = 0, 0, 0
    for n, (op, ln) in enumerate(ops):
        if op == M:
            nm += sum(1 for d in range(ln) if Q[x + d] != T[y + d])
            x += ln; y += ln
        elif op == I:
            nm += ln; x += ln
        else:
            if 0 < n < len(ops) - 1:
                nm += ln
            y += ln
    assert x == len(Q) and y == len(T)
    return nm


def classify(s, r, text_bytes, qer_bytes, L):
    """1 aligned, 0 rid = -1 by the rules, -1 a range outside its arena (rid = -1 on the device, an error of the host entry)."""
    lq, qb, qe = int(s["lq"]), int(r["qb"]), int(r["qe"])
    rb, re = int(s["roff"]) + int(r["rb"]), int(s["roff"]) + int(r["re"])
    if qb < 0 or qe <= qb or rb >= re or rb < L < re:
        return 0
    if lq < 0 or int(s["qoff"]) < 0 or int(s["qoff"]) + lq > qer_bytes or qe > lq or rb < 0 or re > min(text_bytes, 2 * L):
        return -1
    return 1


def record(p, s, r, text, qer, L, contig_off, lookup=global_rolling, detail=None):
    """One record -> (dict of the gbx_mem_aln fields but cigar_off, [CIGAR words])."""
    none = dict(pos=0, rid=-1, is_rev=0, n_cigar=0, nm=0, score=0, w=0, tries=0)
    if classify(s, r, len(text), len(qer), L) != 1:
        return none, []
    lq, qb, qe = int(s["lq"]), int(r["qb"]), int(r["qe"])
    rb, re = int(s["roff"]) + int(r["rb"]), int(s["roff"]) + int(r["re"])
    truesc, rw, a, w = int(r["truesc"]), int(r["w"]), p["mat"][0], p["w"]
    read = [min(int(c), 4) for c in qer[int(s["qoff"]):int(s["qoff"]) + lq]]
    Q, T = read[qb:qe], [min(int(c), 4) for c in text[rb:re]]
    is_rev = 1 if rb >= L else 0
    if is_rev:
        Q, T = Q[::-1], T[::-1]
    w2 = first_band(p, qe - qb, re - rb, truesc, rw)
    last, tries = -(1 << 30), 0
    for i in range(3):
        w2 = min(w2, 4 * w)
        score, ops, wb = gen(p, Q, T, w2, lookup)
        tries, used = tries + 1, w2
        if score == last or w2 == 4 * w:
            break
        last = score
        w2 <<= 1
        if not (i + 1 < 3 and score < truesc - a):
            break
    nm = count_nm(ops, Q, T)
    pos = 2 * L - re if is_rev else rb
    squeezed = 0
    if ops[0][0] == D:
        pos += ops[0][1]
        squeezed = ops[0][1]
        ops = ops[1:]
    elif ops[-1][0] == D:
        squeezed = ops[-1][1]
        ops = ops[:-1]
    rid = max(c for c in range(len(contig_off) - 1) if contig_off[c] <= pos)
    clip5, clip3 = (lq - qe, qb) if is_rev else (qb, lq - qe)
    words = ([[S, clip5]] if clip5 else []) + ops + ([[S, clip3]] if clip3 else [])
    if detail is not None:
        detail.update(Q=Q, T=T, ops=ops, squeezed=squeezed, wb=wb, clip5=clip5, clip3=clip3)
    return (dict(pos=pos - int(contig_off[rid]), rid=rid, is_rev=is_rev, n_cigar=len(words), nm=nm, score=score, w=used, tries=tries),
            [ln << 4 | op for op, ln in words])


def run(p, seeds, res, text, qer, L, contig_off, lookup=global_rolling):
    """Every record -> (alns ALN_DTYPE[n], cigar uint32[total])."""
    res = np.ascontiguousarray(res).view(RESULT_DTYPE).reshape(-1)
    alns, cigar = np.zeros(len(seeds), dtype=ALN_DTYPE), []
    for k in range(len(seeds)):
        a, words = record(p, seeds[k], res[k], text, qer, L, [int(c) for c in contig_off], lookup)
        for f, v in a.items():
            alns[k][f] = v
        alns[k]["cigar_off"] = len(cigar)
        cigar += words
    return alns, np.array(cigar, dtype=np.uint32)


# ---- the C twin ----------------------------------------------------------------------------------------------------
class CParams(C.Structure):
    _fields_ = [("mat", C.c_int32 * 25), ("o_del", C.c_int32), ("e_del", C.c_int32), ("o_ins", C.c_int32), ("e_ins", C.c_int32),
                ("w", C.c_int32)]


_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


def _L():
    global _lib
    if _lib is None:
        src = os.path.join(_HERE, "mem_cigar_ref.c")
        out = os.path.join(_HERE, "libmem_cigar_ref.so")
        if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
            if not os.access(_HERE, os.W_OK):
                out = os.path.join(tempfile.mkdtemp(prefix="mem_cigar_ref"), "libmem_cigar_ref.so")
            subprocess.run(["cc", "-O2", "-std=c11", "-fPIC", "-shared", src, "-o", out], check=True)
        _lib = C.CDLL(out)
        vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
        _lib.mcr_run.argtypes = [C.POINTER(CParams), i64, vp, vp, vp, i64, vp, i64, i64, i32, vp, vp, vp, i64]
        _lib.mcr_run.restype = i64
    return _lib


def run_c(p, seeds, res, text, qer, L, contig_off):
    """run() by the C twin (the rolling form)."""
    cp = CParams()
    for i, v in enumerate(p["mat"]):
        cp.mat[i] = v
    cp.o_del, cp.e_del, cp.o_ins, cp.e_ins, cp.w = p["o_del"], p["e_del"], p["o_ins"], p["e_ins"], p["w"]
    seeds = np.ascontiguousarray(seeds, dtype=SEED_DTYPE)
    res = np.ascontiguousarray(np.ascontiguousarray(res).view(np.int32).reshape(-1, 8))
    text, qer = np.ascontiguousarray(text, dtype=np.uint8), np.ascontiguousarray(qer, dtype=np.uint8)
    co = np.ascontiguousarray(contig_off, dtype=np.int64)
    n = len(seeds)
    alns = np.zeros(max(n, 1), dtype=ALN_DTYPE)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    cap = 64
    while True:
        cigar = np.zeros(cap, dtype=np.uint32)
        got = _L().mcr_run(C.byref(cp), n, ptr(seeds), ptr(res), ptr(text), text.size, ptr(qer), qer.size, int(L), len(co) - 1, ptr(co),
                           ptr(alns), ptr(cigar), cap)
        if got <= cap:
            return alns[:n], cigar[:got]
        cap = int(got)
