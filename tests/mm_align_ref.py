"""Plain restatement of the base-level alignment rules: sequential, full matrices, as close to the rule text as it
can be.  tests/mm_align_ref.c is its C twin for the sizes Python cannot do in a few seconds."""
import math

NEG = -math.inf
LEFT, RIGHT = 0, 1
DEFAULTS = dict(a=2, b=4, sc_ambi=1, q=4, e=2, q2=24, e2=1, bw=500, zdrop=400, end_bonus=0, min_ksw_len=200, max_ext=5000)
ALN_FIELDS = ("rs", "re", "qs", "qe", "mlen", "blen", "n_ambi", "nm", "dp_score", "dp_max", "n_cigar", "flags", "cigar_off")
OPS = "MID"


def params(**kw):
    p = dict(DEFAULTS)
    for k, v in kw.items():
        assert k in p, k
        p[k] = v
    return p


def code(ch):
    """a byte -> 0..3 for A C G T in either case, else 4"""
    return {65: 0, 67: 1, 71: 2, 84: 3}.get(ch & 0xdf, 4)


def codes(s):
    return [code(c) for c in (s.encode() if isinstance(s, str) else bytes(s))]


def sc(P, t, c):
    return -P["sc_ambi"] if t > 3 or c > 3 else P["a"] if t == c else -P["b"]


def gap(P, l):
    return min(P["q"] + P["e"] * l, P["q2"] + P["e2"] * l)


def in_band(t, j, w):
    r = t + j
    return (r - w + 1) >> 1 <= t <= (r + w) >> 1


def dp_job(P, T, Q, w, mode, ext, stats=None):
    """One DP job on code lists T, Q (both at least 1 long) -> dict(score, end=(t, j) or None, zdropped, reach_end, ops=[(op, len)] in
    the job's direction, ct, cq).  op: 0 M, 1 I, 2 D."""
    tl, ql = len(T), len(Q)
    assert tl >= 1 and ql >= 1 and w >= 1
    q, e, q2, e2 = P["q"], P["e"], P["q2"], P["e2"]
    take = (lambda c, z: c >= z) if mode == RIGHT else (lambda c, z: c > z)
    H, G, D = {}, {}, {}                                          # (t, j) -> H; (t, j) -> [E, F, E2, F2]; (t, j) -> (d, flags)
    H[(-1, -1)] = 0
    for j in range(ql):
        H[(-1, j)] = -gap(P, j + 1)
    for t in range(tl):
        H[(t, -1)] = -gap(P, t + 1)
    getH = lambda t, j: H.get((t, j), NEG)
    getG = lambda t, j, k: G[(t, j)][k] if (t, j) in G else NEG   # gap states on a border and outside the band: minus infinity
    mx, mx_t, mx_q, mqe, mqe_t, zdropped, worst = 0, -1, -1, NEG, -1, False, 0
    for r in range(tl + ql - 1):
        cells = [t for t in range(max(0, r - ql + 1), min(tl - 1, r) + 1) if in_band(t, r - t, w)]
        for t in cells:
            j = r - t
            st, fl = [], []
            for k, (pt, pj, qq, ee) in enumerate(((t - 1, j, q, e), (t, j - 1, q, e), (t - 1, j, q2, e2), (t, j - 1, q2, e2))):
                opened, ext_ = getH(pt, pj) - qq, getG(pt, pj, k)
                border = pt < 0 or pj < 0
                fl.append((not border) and (ext_ >= opened if mode == RIGHT else ext_ > opened))
                st.append(max(opened, ext_) - ee)
            z, d = getH(t - 1, j - 1) + sc(P, T[t], Q[j]), 0
            for k in range(4):
                if take(st[k], z):
                    z, d = st[k], k + 1
            H[(t, j)], G[(t, j)], D[(t, j)] = z, st, (d, fl)
        if not ext or not cells:
            continue
        best, bt = max((H[(t, r - t)], -t) for t in cells)
        bt = -bt
        for t in cells:
            if r - t == ql - 1 and H[(t, r - t)] > mqe:
                mqe, mqe_t = H[(t, r - t)], t
        if best > mx:
            mx, mx_t, mx_q = best, bt, r - bt
        elif bt >= mx_t and r - bt >= mx_q:
            l = abs((bt - mx_t) - ((r - bt) - mx_q))
            if P["zdrop"] >= 0 and mx - best > P["zdrop"] + l * e2:
                zdropped = True
                break
            worst = max(worst, mx - best)
    if stats is not None and ext and not zdropped and 0 <= P["zdrop"] < worst:
        stats["saved_by_l"] = stats.get("saved_by_l", 0) + 1      # a drop that only the l e2 term held off
    reach = False
    if not ext:
        end, score = (tl - 1, ql - 1), H[(tl - 1, ql - 1)]
    elif not zdropped and mqe + P["end_bonus"] > mx:
        end, score, reach = (mqe_t, ql - 1), mqe, True
    elif mx_t >= 0:
        end, score = (mx_t, mx_q), mx
    else:
        end, score = None, 0
    ops = []
    if end is not None:
        i, j = end
        state = 0
        while i >= 0 and j >= 0:
            d, fl = D[(i, j)]
            if state == 0:
                state = d
            if state == 0:
                ops.append(0)
                i, j = i - 1, j - 1
            elif state in (1, 3):
                ops.append(2)
                i -= 1
                if not fl[state - 1]:
                    state = 0
            else:
                ops.append(1)
                j -= 1
                if not fl[state - 1]:
                    state = 0
        ops += [2] * (i + 1) + [1] * (j + 1)
        ops.reverse()
    return dict(score=score, end=end, zdropped=zdropped, reach_end=reach, ops=merge([(o, 1) for o in ops]),
                ct=0 if end is None else end[0] + 1, cq=0 if end is None else end[1] + 1)


def merge(runs):
    out = []
    for o, l in runs:
        if l <= 0:
            continue
        if out and out[-1][0] == o:
            out[-1] = (o, out[-1][1] + l)
        else:
            out.append((o, l))
    return out


def rescore(P, T, Q, ops):
    """the score of a job's runs over its sequences and what they consume"""
    s = t = j = 0
    for o, l in ops:
        if o == 0:
            s += sum(sc(P, T[t + k], Q[j + k]) for k in range(l))
            t, j = t + l, j + l
        else:
            s -= gap(P, l)
            if o == 2:
                t += l
            else:
                j += l
    return s, t, j


def general_gap_global(P, T, Q):
    """An independent global DP with the general gap cost gap(l): O(n^3), for small inputs"""
    tl, ql = len(T), len(Q)
    H = [[NEG] * (ql + 1) for _ in range(tl + 1)]
    H[0][0] = 0
    for i in range(tl + 1):
        for j in range(ql + 1):
            if i == 0 and j == 0:
                continue
            b = NEG
            if i and j:
                b = H[i - 1][j - 1] + sc(P, T[i - 1], Q[j - 1])
            for l in range(1, i + 1):
                b = max(b, H[i - l][j] - gap(P, l))
            for l in range(1, j + 1):
                b = max(b, H[i][j - l] - gap(P, l))
            H[i][j] = b
    return H[tl][ql]


def oriented(read, rev):
    c = codes(read)
    return [3 - x if x < 4 else 4 for x in reversed(c)] if rev else c


def plan(P, xs, tlen, qlen, stats=None):
    """rules 2-5: the anchors' (x, y, span) -> [(kind, t0, q0, tl, ql, w)], kind 0 left, 1 fill, 2 right"""
    x0, y0, s0 = xs[0]
    rs, qs = x0 + 1 - s0, y0 + 1 - s0
    re, qe = rs, qs
    jobs = []
    lq = min(qs, P["max_ext"])
    lt = min(rs, lq + P["bw"])
    jobs.append((0, rs - lt, qs - lq, lt, lq, P["bw"]) if lq > 0 and lt > 0 else (0, rs, qs, 0, 0, P["bw"]))
    for i in range(1, len(xs)):
        x, y, sp = xs[i]
        if stats is not None and (x - (sp >> 1) < rs or y - (sp >> 1) < qs):
            stats["clamped"] = stats.get("clamped", 0) + 1
        re, qe = max(x - (sp >> 1), rs), max(y - (sp >> 1), qs)
        if i == len(xs) - 1 or (re - rs >= P["min_ksw_len"] and qe - qs >= P["min_ksw_len"]):
            jobs.append((1, rs, qs, re - rs, qe - qs, max(P["bw"], abs((re - rs) - (qe - qs)) + 1)))
            if stats is not None:
                stats["fills"] = stats.get("fills", 0) + 1
            rs, qs = re, qe
    lq = min(qlen - qe, P["max_ext"])
    lt = min(tlen - re, lq + P["bw"])
    jobs.append((2, re, qe, lt, lq, P["bw"]) if lq > 0 and lt > 0 else (2, re, qe, 0, 0, P["bw"]))
    return jobs


def ring(w, tl):
    """the ints of a DP row: the power of two that holds a diagonal's band and three more"""
    need, m = min(min(w, 1 << 40) + 1, tl) + 3, 4
    while m < need:
        m <<= 1
    return m


def job_bytes(w, tl, ql):
    """the bytes of z a DP job takes (layout): eleven rows of M ints and a direction byte a cell slot"""
    w = min(w, tl + ql)
    return (11 * 4 * ring(w, tl) + (tl + ql - 1) * min(w + 1, tl, ql) + 15) & ~15


def copy_record(g, flags):
    return dict(rs=g["rs"], re=g["re"], qs=g["qs"], qe=g["qe"], mlen=g["mlen"], blen=g["blen"], n_ambi=0, nm=0, dp_score=0, dp_max=0, n_cigar=0,
                flags=flags, cigar_off=0)


def align_region(P, g, anchors, n_chained, T, read, n_targets, stats=None, dp=None):
    """One region -> (record without cigar_off, words, jobs, z bytes) or (record, None, 0, 0) when invalid.  g: dict of the
    gbx_mm_reg fields; anchors: the read's chained (ax, ay) pairs; T: the contig's codes or None; read: bytes."""
    qlen = len(read)
    bad = not (0 <= g["rid"] < n_targets) or g["cnt"] < 1 or g["as"] < 0 or g["as"] + g["cnt"] > n_chained
    xs = []
    if not bad:
        for ax, ay in anchors[g["as"]:g["as"] + g["cnt"]]:
            x, y = ax & 0xffffffff, ay & 0xffffffff
            xs.append((x - (1 << 32) if x >> 31 else x, y - (1 << 32) if y >> 31 else y, ay >> 32 & 0xff))
        tlen = len(T)
        bad = xs[0][0] + 1 - xs[0][2] < 0 or xs[0][1] + 1 - xs[0][2] < 0 or any(x < 0 or y < 0 or x >= tlen or y >= qlen for x, y, _ in xs)
    if bad:
        return copy_record(g, 64), None, 0, 0
    Q = oriented(read, g["rev"])
    jobs = plan(P, xs, tlen, qlen, stats)
    dp = dp or dp_job
    zb = sum(job_bytes(w, tl, ql) for _, _, _, tl, ql, w in jobs if tl > 0 and ql > 0)
    runs, score, fl = [], 0, 1
    rs = re = qs = qe = None
    for kind, t0, q0, tl, ql, w in jobs:
        if kind == 1:
            if tl > 0 and ql > 0:
                r = dp(P, T[t0:t0 + tl], Q[q0:q0 + ql], w, LEFT, False)
                score += r["score"]
                runs += r["ops"]
            elif tl or ql:
                score -= gap(P, tl or ql)
                runs.append((2 if tl else 1, tl or ql))
            continue
        ct = cq = 0
        if tl > 0 and ql > 0:
            if kind == 0:
                r = dp(P, T[t0:t0 + tl][::-1], Q[q0:q0 + ql][::-1], w, RIGHT, True, stats)
                runs += r["ops"][::-1]
            else:
                r = dp(P, T[t0:t0 + tl], Q[q0:q0 + ql], w, LEFT, True, stats)
                runs += r["ops"]
            score += r["score"]
            ct, cq = r["ct"], r["cq"]
            fl |= (2 if kind == 0 else 4) * r["zdropped"] | (8 if kind == 0 else 16) * r["reach_end"]
            if stats is not None:
                for k in ("zdropped", "reach_end"):
                    stats[k] = stats.get(k, 0) + r[k]
                stats["empty_ext"] = stats.get("empty_ext", 0) + (r["end"] is None)
        if kind == 0:
            rs, qs = t0 + tl - ct, q0 + ql - cq
        else:
            re, qe = t0 + ct, q0 + cq
    words = merge(runs)
    mlen = blen = amb = s = mx = 0
    t, j = rs, qs
    for o, l in words:
        assert l < 1 << 28
        if o == 0:
            for k in range(l):
                tc, qc = T[t + k], Q[j + k]
                if tc > 3 or qc > 3:
                    amb += 1
                elif tc == qc:
                    mlen, blen = mlen + 1, blen + 1
                else:
                    blen += 1
                s += sc(P, tc, qc)
                if s < 0:
                    s = 0
                else:
                    mx = max(mx, s)
            t, j = t + l, j + l
        else:
            k = sum(c > 3 for c in (T[t:t + l] if o == 2 else Q[j:j + l]))
            blen, amb = blen + l - k, amb + k
            s = max(0, s - gap(P, l))
            if o == 2:
                t += l
            else:
                j += l
    assert (t, j) == (re, qe), "the CIGAR does not consume the reported spans"
    rec = dict(rs=rs, re=re, qs=qlen - qe if g["rev"] else qs, qe=qlen - qs if g["rev"] else qe, mlen=mlen, blen=blen, n_ambi=amb, nm=blen - mlen + amb,
               dp_score=score, dp_max=mx, n_cigar=len(words), flags=fl, cigar_off=0)
    return rec, [l << 4 | o for o, l in words], len(jobs), zb


def align_batch(P, regs, reg_off, off, cax, cay, n_chained, reads, refs, z_bytes=None, stats=None, dp=None):
    """The call -> dict(alns=[record], cigar=[word], counts=(jobs, words, z bytes)).  regs: list of dicts; reads, refs: bytes.
    z_bytes None: room for everything.  dp: what runs a DP job (dp_job; the tests pass the C twin for the larger cases)."""
    ref_codes = [codes(r) for r in refs]
    alns, cigar, n_jobs, z_need = [], [], 0, 0
    for r in range(len(reads)):
        anchors = [(int(cax[i]), int(cay[i])) for i in range(int(off[r]), int(off[r]) + int(n_chained[r]))]
        for gi in range(int(reg_off[r]), int(reg_off[r + 1])):
            g = regs[gi]
            T = ref_codes[g["rid"]] if 0 <= g["rid"] < len(refs) else None
            rec, words, nj, zb = align_region(P, g, anchors, int(n_chained[r]), T, reads[r], len(refs), stats, dp)
            n_jobs += nj
            z_need += zb
            if words is not None and z_bytes is not None and z_need > z_bytes:
                rec, words = copy_record(g, 32), None
            if words is not None:
                rec["cigar_off"] = len(cigar)
                cigar += words
            alns.append(rec)
    return dict(alns=alns, cigar=cigar, counts=(n_jobs, len(cigar), z_need))


def cigar_text(words):
    return "".join("%d%s" % (w >> 4, OPS[w & 15]) for w in words)


def paf_cigar(regs, reg_off, alns, cigar, qnames, qlen, tnames, tlen, rep_len):
    """rule 9 -> the text.  regs: dict of arrays or list of dicts, as mm_map_ref.paf takes its regions"""
    import mm_map_ref as MR
    out = []
    for r in range(len(reg_off) - 1):
        for gi in range(int(reg_off[r]), int(reg_off[r + 1])):
            g = {k: int(regs[k][gi]) for k in MR.REG_FIELDS} if isinstance(regs, dict) else regs[gi]
            a = alns[gi]
            ok = 0 <= g["rid"] < len(tnames)
            if not (a["flags"] & 1) or a["flags"] & 96:
                out.append(MR.paf_line(g, qnames[r], int(qlen[r]), tnames[g["rid"]] if ok else "*", int(tlen[g["rid"]]) if ok else 0, int(rep_len[r])))
                continue
            f = [qnames[r], qlen[r], a["qs"], a["qe"], "-" if g["rev"] else "+", tnames[g["rid"]] if ok else "*", tlen[g["rid"]] if ok else 0, a["rs"], a["re"],
                 a["mlen"], a["blen"], g["mapq"], "NM:i:%d" % a["nm"], "ms:i:%d" % a["dp_max"], "AS:i:%d" % a["dp_score"], "nn:i:%d" % a["n_ambi"],
                 "tp:A:" + ("P" if g["parent"] == g["id"] else "S"), "cm:i:%d" % g["cnt"], "s1:i:%d" % g["score"]]
            if g["parent"] == g["id"]:
                f.append("s2:i:%d" % g["subsc"])
            f += ["rl:i:%d" % rep_len[r], "cg:Z:" + cigar_text(cigar[a["cigar_off"]:a["cigar_off"] + a["n_cigar"]])]
            out.append("\t".join(str(x) for x in f) + "\n")
    return "".join(out)


# ---- the C twin of dp_job (tests/mm_align_ref.c, built on first use)
_lib = None


def _L():
    global _lib
    if _lib is None:
        import ctypes as C
        import os
        import subprocess
        import tempfile
        here = os.path.dirname(os.path.abspath(__file__))
        src, out = os.path.join(here, "mm_align_ref.c"), os.path.join(here, "libmm_align_ref.so")
        if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
            if not os.access(here, os.W_OK):
                out = os.path.join(tempfile.mkdtemp(prefix="mm_align_ref"), "libmm_align_ref.so")
            subprocess.run(["cc", "-O2", "-std=c11", "-fPIC", "-shared", src, "-o", out], check=True)
        _lib = C.CDLL(out)
        _lib.mar_job.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.c_char_p, C.c_int32, C.c_int32, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64]
        _lib.mar_job.restype = C.c_int64
    return _lib


def dp_job_c(P, T, Q, w, mode, ext, stats=None):
    """dp_job by the C twin: the same dict"""
    import ctypes as C
    pv = (C.c_int32 * 12)(*[P[k] for k in ("a", "b", "sc_ambi", "q", "e", "q2", "e2", "bw", "zdrop", "end_bonus", "min_ksw_len", "max_ext")])
    out, cap = (C.c_int32 * 8)(), len(T) + len(Q) + 1
    ops = (C.c_int32 * (2 * cap))()
    n = _L().mar_job(pv, bytes(T), len(T), bytes(Q), len(Q), min(w, len(T) + len(Q)), mode, int(ext), out, ops, cap)
    assert 0 <= n <= cap
    if stats is not None and out[7]:
        stats["saved_by_l"] = stats.get("saved_by_l", 0) + 1
    return dict(score=out[0], end=None if out[1] < 0 else (out[1], out[2]), zdropped=bool(out[3]), reach_end=bool(out[4]),
                ops=[(ops[2 * k], ops[2 * k + 1]) for k in range(n)], ct=out[5], cq=out[6])
