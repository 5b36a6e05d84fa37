"""A sequential restatement of the mm sam rules: SAM records, cs / MD tags and = / X CIGAR operations of aligned
regions, and validate(), which checks a SAM text against the reads and contigs alone.  Neither shares code with the product, and
validate() shares none with the restatement.  UPSTREAM-KNOWLEDGE: after minimap2's mm_write_sam3, write_cs_core, write_MD_core
and mm_update_cigar_eqx as published.

Records are dicts: a region has the fields of gbx_mm_reg, an alignment those of gbx_mm_aln."""
import re

OPS = "MIDNSHP=X"
_COMP = bytes.maketrans(b"ACGTUMRWSYKVHDBNacgtumrwsykvhdbn", b"TGCAAKYWSRMBDHVNtgcaakywsrmbdhvn")


def params(**kw):
    p = dict(format=0, cs=0, md=0, eqx=0, softclip=0)
    assert set(kw) <= set(p)
    p.update(kw)
    return p


def code(b):
    return {65: 0, 67: 1, 71: 2, 84: 3}.get(b & 0xdf, 4)


def oriented(read, rev):
    return bytes(read)[::-1].translate(_COMP) if rev else bytes(read)


def prints(a, n_cigar):
    """the region prints its alignment"""
    return bool(a["flags"] & 1) and not a["flags"] & (32 | 64) and a["n_cigar"] >= 0 and a["cigar_off"] >= 0 and a["cigar_off"] + a["n_cigar"] <= n_cigar


def clips(a, rev, qlen):
    s, e = (qlen - a["qe"], qlen - a["qs"]) if rev else (a["qs"], a["qe"])
    s = min(max(s, 0), qlen)
    e = min(max(e, s), qlen)
    return s, qlen - e


def columns(words, t, q, tlen, qlen):
    """[(op, len, n, t, q)]: n the columns a word counts from column t of the contig and q of the oriented read"""
    out = []
    for w in words:
        op, ln = w & 15, w >> 4
        n = ln
        if op in (0, 2):
            n = min(n, tlen - t)
        if op in (0, 1):
            n = min(n, qlen - q)
        if op > 2:
            n = 0
        out.append((op, ln, n, t, q))
        if op in (0, 2):
            t += n
        if op in (0, 1):
            q += n
    return out


def letter(op):
    return OPS[op] if op < 9 else "?"


def cigar_text(cols, T, Q, eqx):
    if not eqx:
        return "".join("%d%s" % (ln, letter(op)) for op, ln, _, _, _ in cols)
    out = []
    for op, ln, n, t, q in cols:
        if op != 0:
            out.append("%d%s" % (ln, letter(op)))
            continue
        run, kind = 0, None
        for i in range(n):
            k = "=" if code(T[t + i]) == code(Q[q + i]) else "X"
            if k != kind and run:
                out.append("%d%s" % (run, kind))
                run = 0
            kind, run = k, run + 1
        if run:
            out.append("%d%s" % (run, kind))
    return "".join(out)


def cs_text(cols, T, Q, form):
    out = []
    for op, _, n, t, q in cols:
        if n <= 0:
            continue
        if op == 1:
            out.append("+" + "".join("acgtn"[code(b)] for b in Q[q:q + n]))
        elif op == 2:
            out.append("-" + "".join("acgtn"[code(b)] for b in T[t:t + n]))
        else:
            run = []
            for i in range(n + 1):
                eq = i < n and code(T[t + i]) == code(Q[q + i])
                if eq:
                    run.append("ACGTN"[code(Q[q + i])])
                    continue
                if run:
                    out.append(":%d" % len(run) if form == 1 else "=" + "".join(run))
                    run = []
                if i < n:
                    out.append("*" + "acgtn"[code(T[t + i])] + "acgtn"[code(Q[q + i])])
    return "".join(out)


def md_text(cols, T, Q):
    out, c = [], 0
    for op, _, n, t, q in cols:
        if n <= 0 or op == 1:
            continue
        if op == 2:
            out.append("%d^%s" % (c, "".join("ACGTN"[code(b)] for b in T[t:t + n])))
            c = 0
            continue
        for i in range(n):
            if code(T[t + i]) == code(Q[q + i]):
                c += 1
            else:
                out.append("%d%s" % (c, "ACGTN"[code(T[t + i])]))
                c = 0
    if c > 0:
        out.append("%d" % c)
    return "".join(out)


def tags(g, a, rep):
    out = ["NM:i:%d" % a["nm"], "ms:i:%d" % a["dp_max"], "AS:i:%d" % a["dp_score"], "nn:i:%d" % a["n_ambi"], "tp:A:" + ("P" if g["parent"] == g["id"] else "S"),
           "cm:i:%d" % g["cnt"], "s1:i:%d" % g["score"]]
    if g["parent"] == g["id"]:
        out.append("s2:i:%d" % g["subsc"])
    return out + ["rl:i:%d" % rep]


def sam_text(P, regs, reg_off, alns, cigar, qnames, reads, quals, rep_len, tnames, refs):
    """-> dict(text bytes, line_off, counts = (lines, regions that print nothing))"""
    out, line_off, n_lines, n_silent = [], [], 0, 0
    at = 0
    nm = lambda s: s.decode() if isinstance(s, bytes) else s
    for r in range(len(reg_off) - 1):
        line_off.append(at)
        read, qlen, qname = bytes(reads[r]), len(reads[r]), nm(qnames[r])
        gs = list(range(reg_off[r], reg_off[r + 1]))
        ok = {g: regs[g]["read"] == r and prints(alns[g], len(cigar)) for g in gs}
        own = [g for g in gs if ok[g] and regs[g]["parent"] == regs[g]["id"]]
        for g in gs:
            reg, a = regs[g], alns[g]
            if reg["read"] != r:
                n_silent += 1
                continue
            tok = 0 <= reg["rid"] < len(refs)
            T, tname = (bytes(refs[reg["rid"]]), nm(tnames[reg["rid"]])) if tok else (b"", "*")
            Q = oriented(read, reg["rev"])
            if ok[g]:
                c5, c3 = clips(a, reg["rev"], qlen)
                words = cigar[a["cigar_off"]:a["cigar_off"] + a["n_cigar"]]
                cols = columns([int(w) for w in words], min(max(a["rs"], 0), len(T)), c5, len(T), qlen)
                extra = []
                if P["cs"]:
                    extra.append("cs:Z:" + cs_text(cols, T, Q, P["cs"]))
                if P["md"]:
                    extra.append("MD:Z:" + md_text(cols, T, Q))
            if P["format"] == 0:
                if ok[g]:
                    f = [qname, qlen, a["qs"], a["qe"], "-" if reg["rev"] else "+", tname, len(T), a["rs"], a["re"], a["mlen"], a["blen"], reg["mapq"]]
                    f += tags(reg, a, rep_len[r]) + ["cg:Z:" + cigar_text(cols, T, Q, P["eqx"])] + extra
                else:
                    f = [qname, qlen, reg["qs"], reg["qe"], "-" if reg["rev"] else "+", tname, len(T), reg["rs"], reg["re"], reg["mlen"], reg["blen"], reg["mapq"],
                         "tp:A:" + ("P" if reg["parent"] == reg["id"] else "S"), "cm:i:%d" % reg["cnt"], "s1:i:%d" % reg["score"]]
                    if reg["parent"] == reg["id"]:
                        f.append("s2:i:%d" % reg["subsc"])
                    f.append("rl:i:%d" % rep_len[r])
                line = "\t".join(str(x) for x in f) + "\n"
            elif not ok[g]:
                n_silent += 1
                continue
            else:
                is_own = reg["parent"] == reg["id"]
                secondary, supp = not is_own, is_own and g != own[0]
                hard = (secondary or supp) and not P["softclip"]
                cl = "H" if hard else "S"
                cg = ("%d%s" % (c5, cl) if c5 > 0 else "") + cigar_text(cols, T, Q, P["eqx"]) + ("%d%s" % (c3, cl) if c3 > 0 else "")
                qual = None if quals is None else (bytes(quals[r])[::-1] if reg["rev"] else bytes(quals[r]))
                if secondary:
                    seq, ql = "*", "*"
                else:
                    lo, hi = (c5, qlen - c3) if hard else (0, qlen)
                    seq, ql = Q[lo:hi].decode("latin-1"), "*" if qual is None else qual[lo:hi].decode("latin-1")
                f = [qname, (0x10 if reg["rev"] else 0) | (0x100 if secondary else 0) | (0x800 if supp else 0), tname, a["rs"] + 1, reg["mapq"], cg, "*", 0, 0, seq, ql]
                f += tags(reg, a, rep_len[r])
                if is_own and len(own) >= 2:
                    sa = []
                    for h in own:
                        if h == g:
                            continue
                        o, og = alns[h], regs[h]
                        o5, o3 = clips(o, og["rev"], qlen)
                        lq, lt = o["qe"] - o["qs"], o["re"] - o["rs"]
                        summ = ("%dS" % o5 if o5 > 0 else "") + "%dM" % min(lq, lt) + ("%dI" % (lq - lt) if lq > lt else "") + ("%dD" % (lt - lq) if lt > lq else "") + \
                               ("%dS" % o3 if o3 > 0 else "")
                        on = nm(tnames[og["rid"]]) if 0 <= og["rid"] < len(refs) else "*"
                        sa.append("%s,%d,%s,%s,%d,%d;" % (on, o["rs"] + 1, "-" if og["rev"] else "+", summ, og["mapq"], o["nm"]))
                    f.append("SA:Z:" + "".join(sa))
                line = "\t".join(str(x) for x in f + extra) + "\n"
            out.append(line)
            n_lines += 1
            at += len(line.encode("latin-1"))
        if P["format"] == 1 and not any(ok.values()):
            ql = "*" if quals is None else bytes(quals[r]).decode("latin-1")
            line = "\t".join([qname, "4", "*", "0", "0", "*", "*", "0", "0", read.decode("latin-1"), ql]) + "\n"
            out.append(line)
            n_lines += 1
            at += len(line.encode("latin-1"))
    line_off.append(at)
    return dict(text="".join(out).encode("latin-1"), line_off=line_off, counts=(n_lines, n_silent))


# ---------------------------------------------------------------------------------------------------------------- the validator
class Invalid(AssertionError):
    pass


def _need(ok, what, line):
    if not ok:
        raise Invalid("%s: %s" % (what, line[:200]))


def _c(b):
    u = chr(b).upper() if isinstance(b, int) else b.upper()
    return "ACGT".find(u) if u in "ACGT" else 4


def _rc(s):
    pairs = dict(zip("ACGTUMRWSYKVHDBN", "TGCAAKYWSRMBDHVN"))
    pairs.update({k.lower(): v.lower() for k, v in pairs.items()})
    return "".join(pairs.get(ch, ch) for ch in reversed(s))


def validate(text, reads, refs, line_off=None):
    """Every SAM record of `text` (str, no header needed) against reads = [(name, sequence)] and refs = [(name, sequence)] (str):
    the contig stretch at POS rebuilt from SEQ + CIGAR + MD and again from cs, both equal to the contig as codes; every = / X against
    its columns; NM; the CIGAR's query length with the H clips; line_off, when given, tiles the text a read at a time.
    -> the number of records checked.  Raises Invalid."""
    lines = text.split("\n")
    _need(lines[-1] == "", "the text does not end in a newline", text[-50:])
    lines = [ln for ln in lines[:-1] if not ln.startswith("@")]
    by_name = {}
    for name, s in reads:
        by_name.setdefault(name, s)
    contig = dict(refs)
    if line_off is not None:
        body = "".join(ln + "\n" for ln in lines)
        _need(line_off[0] == 0 and line_off[-1] == len(body) and len(line_off) == len(reads) + 1, "line_off does not span the text", str(list(line_off)[:8]))
        for r, (name, _) in enumerate(reads):
            lo, hi = line_off[r], line_off[r + 1]
            _need(lo <= hi and (lo == 0 or body[lo - 1] == "\n"), "line_off is not at a line start", str(lo))
            for ln in body[lo:hi].split("\n")[:-1]:
                _need(ln.split("\t")[0] == name, "a line outside its read's range", ln)
    checked = 0
    for ln in lines:
        f = ln.split("\t")
        _need(len(f) >= 11, "fewer than 11 fields", ln)
        flag = int(f[1])
        read = by_name[f[0]]
        if flag & 4:
            _need(f[9] == read and f[2] == "*" and f[5] == "*", "an unmapped record", ln)
            continue
        tag = {t[:2]: t[5:] for t in f[11:]}
        T = contig[f[2]]
        pos = int(f[3]) - 1
        ops = [(int(n), o) for n, o in re.findall(r"(\d+)([MIDNSHP=X])", f[5])]
        _need("".join("%d%s" % x for x in ops) == f[5], "a CIGAR that does not parse", ln)
        Q = _rc(read) if flag & 16 else read
        h5 = ops[0][0] if ops and ops[0][1] == "H" else 0
        h3 = ops[-1][0] if len(ops) > 1 and ops[-1][1] == "H" else 0
        qsum = sum(n for n, o in ops if o in "MIS=X")
        _need(qsum + h5 + h3 == len(read), "the CIGAR's query length and H clips are not qlen", ln)
        if f[9] != "*":
            _need(f[9] == Q[h5:len(Q) - h3], "SEQ is not the oriented read between the hard clips", ln)
            if f[10] != "*":
                _need(len(f[10]) == len(f[9]), "QUAL and SEQ differ in length", ln)
        seq = Q[h5:len(Q) - h3]
        # the columns from CIGAR over seq and the contig
        q, t, cols, nm = 0, pos, [], 0
        for n, o in ops:
            if o == "S":
                q += n
            elif o in "M=X":
                for i in range(n):
                    _need(t + i < len(T) and q + i < len(seq), "an alignment past an end", ln)
                    eq = _c(T[t + i]) == _c(seq[q + i])
                    if o != "M":
                        _need(eq == (o == "="), "an = / X that does not match its column", ln)
                    nm += (not eq) or _c(T[t + i]) == 4
                cols.append(("M", t, q, n))
                t += n
                q += n
            elif o == "I":
                cols.append(("I", t, q, n))
                q += n
                nm += n
            elif o == "D":
                cols.append(("D", t, q, n))
                t += n
                nm += n
        want = [_c(ch) for ch in T[pos:t]]
        if "NM" in tag:
            _need(int(tag["NM"]) == nm, "NM is not the columns' count (%d)" % nm, ln)
        if "MD" in tag:
            md = re.findall(r"(\d+)|\^([A-Z]+)|([A-Z])", tag["MD"])
            _need("".join(a or ("^" + b if b else c) for a, b, c in md) == tag["MD"], "an MD that does not parse", ln)
            subst, k = {}, 0                                   # aligned M column index -> contig letter; deletions in order
            dels = []
            for a, b, c in md:
                if a:
                    k += int(a)
                elif b:
                    dels.append(b)
                else:
                    subst[k] = c
                    k += 1
            rebuilt, k, di = [], 0, 0
            for kind, _, q0, n in cols:
                if kind == "M":
                    for i in range(n):
                        rebuilt.append(_c(subst[k]) if k in subst else _c(seq[q0 + i]))
                        k += 1
                elif kind == "D":
                    _need(di < len(dels) and len(dels[di]) == n, "MD's deletions are not the CIGAR's", ln)
                    rebuilt += [_c(ch) for ch in dels[di]]
                    di += 1
            _need(di == len(dels) and all(j < k for j in subst), "MD runs past the alignment", ln)
            _need(rebuilt == want, "SEQ + CIGAR + MD do not rebuild the contig", ln)
            # MD's counts must be the equal runs themselves, not merely something that rebuilds
            exp, c = [], 0
            for kind, t0, q0, n in cols:
                if kind == "M":
                    for i in range(n):
                        if _c(T[t0 + i]) == _c(seq[q0 + i]):
                            c += 1
                        else:
                            exp.append(str(c) + "ACGTN"[_c(T[t0 + i])])
                            c = 0
                elif kind == "D":
                    exp.append(str(c) + "^" + "".join("ACGTN"[_c(ch)] for ch in T[t0:t0 + n]))
                    c = 0
            _need(tag["MD"] == "".join(exp) + (str(c) if c else ""), "MD is not the alignment's", ln)
        if "cs" in tag:
            toks = re.findall(r":(\d+)|=([ACGTN]+)|\*([acgtn])([acgtn])|\+([acgtn]+)|-([acgtn]+)", tag["cs"])
            _need("".join(":" + a if a else "=" + b if b else "*" + c + d if c else "+" + e if e else "-" + g for a, b, c, d, e, g in toks) == tag["cs"],
                  "a cs that does not parse", ln)
            q = ops[0][0] if ops and ops[0][1] == "S" else 0
            rebuilt = []
            for a, b, c, d, e, g in toks:
                if a:
                    rebuilt += [_c(ch) for ch in seq[q:q + int(a)]]
                    q += int(a)
                elif b:
                    _need([_c(ch) for ch in b] == [_c(ch) for ch in seq[q:q + len(b)]], "cs = letters are not the read's", ln)
                    rebuilt += [_c(ch) for ch in b]
                    q += len(b)
                elif c:
                    _need(_c(d) == _c(seq[q]) and _c(c) != _c(d), "a cs substitution that is not the read's", ln)
                    rebuilt.append(_c(c))
                    q += 1
                elif e:
                    _need([_c(ch) for ch in e] == [_c(ch) for ch in seq[q:q + len(e)]], "cs + letters are not the read's", ln)
                    q += len(e)
                else:
                    rebuilt += [_c(ch) for ch in g]
            _need(rebuilt == want, "cs does not rebuild the contig", ln)
            # every equal run maximal within its M word and every column's kind right: compare with the columns
            exp = []
            for kind, t0, q0, n in cols:
                if kind == "M":
                    run = 0
                    for i in range(n + 1):
                        if i < n and _c(T[t0 + i]) == _c(seq[q0 + i]):
                            run += 1
                            continue
                        if run:
                            exp.append((":", run))
                            run = 0
                        if i < n:
                            exp.append(("*", 1))
                else:
                    exp.append(("+" if kind == "I" else "-", n))
            got = [(":", int(a)) if a else (":", len(b)) if b else ("*", 1) if c else ("+", len(e)) if e else ("-", len(g)) for a, b, c, d, e, g in toks]
            _need(got == exp, "cs tokens are not the alignment's", ln)
        checked += 1
    return checked
