"""Hand-built and generated inputs of the CIGAR stage (gbx_mem_cigar_*), shared by the CPU and the GPU tests.

A job is dict(params, L, contig_off, text, qer, seeds, res, names): a two-contig genome, its 2 L-byte text, the reads' arena,
SEED_DTYPE records and the extension results they would have come with (int32[n, 8])."""
import functools
import json
import os

import numpy as np

import mem_cigar_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
L0 = 1600
CONTIGS = [0, 700, L0]


def genome(seed=77, L=L0):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 4, L).astype(np.uint8)
    g[500:510] = 0                                    # a homopolymer, flanked by other bases
    g[499], g[510] = 1, 2
    return g


def text_of(g):
    return np.concatenate([g, (3 - g[::-1]).astype(np.uint8)])


def revcomp(r):
    r = np.asarray(r, dtype=np.uint8)
    return np.where(r[::-1] > 3, r[::-1], 3 - r[::-1]).astype(np.uint8)


class Builder:
    def __init__(self, g=None, contig_off=CONTIGS, **params):
        self.g = genome() if g is None else g
        self.L = len(self.g)
        self.text = text_of(self.g)
        self.params = params
        self.p = R.params(**params)
        self.contig_off = np.array(contig_off, dtype=np.int64)
        self.reads, self.rows, self.names = [], [], []

    def add(self, name, read, g0, g1, rev=False, qb=0, qe=None, truesc=None, rw=100, pad=(7, 9), raw=None):
        """The read (forward-strand sense; stored reverse-complemented when rev) against genome[g0:g1]; [qb, qe) in the
        stored read's coordinates.  raw: result fields set as they are, after everything else."""
        read = np.asarray(read, dtype=np.uint8)
        if rev:
            read = revcomp(read)
        lq = len(read)
        qe = lq if qe is None else qe
        rb, re = (2 * self.L - g1, 2 * self.L - g0) if rev else (g0, g1)
        lo = 0 if not rev else self.L
        roff = max(lo, rb - pad[0])
        rend = min(lo + self.L, re + pad[1])
        if truesc is None:
            Q, T = [int(c) for c in read[qb:qe]], [int(c) for c in self.text[rb:re]]
            truesc = R.global_rolling(Q, T, max(len(Q), len(T)) + 3, self.p)[0] if Q and T else 0
        qoff = sum(len(r) for r in self.reads)
        self.reads.append(read)
        res = dict(score=truesc, truesc=truesc, qb=qb, qe=qe, rb=rb - roff, re=re - roff, w=rw, sc0=0)
        res.update(raw or {})
        self.rows.append((qoff, roff, lq, rend - roff, res))
        self.names.append(name)

    def job(self):
        n = len(self.rows)
        seeds, res = np.zeros(n, dtype=R.SEED_DTYPE), np.zeros(n, dtype=R.RESULT_DTYPE)
        for k, (qoff, roff, lq, rlen, r) in enumerate(self.rows):
            seeds[k]["qoff"], seeds[k]["roff"], seeds[k]["lq"], seeds[k]["rlen"] = qoff, roff, lq, rlen
            seeds[k]["len"] = 1
            for f, v in r.items():
                res[k][f] = v
        qer = np.concatenate(self.reads) if self.reads else np.zeros(0, np.uint8)
        return dict(params=self.params, L=self.L, contig_off=self.contig_off, text=self.text, qer=qer, seeds=seeds,
                    res=res.view(np.int32).reshape(-1, 8), names=list(self.names))


def mutate(piece, subs=(), ins=(), dele=()):
    """piece with substitutions at `subs`, a base inserted before each position of `ins`, the positions of `dele` removed."""
    out = []
    for x, c in enumerate(piece):
        if x in ins:
            out.append((int(c) + 2) % 4)
        if x in dele:
            continue
        out.append((int(c) + 1) % 4 if x in subs else int(c))
    return np.array(out, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def hand_built():
    g = genome()
    J = {}

    b = Builder()
    b.add("perfect", g[100:150], 100, 150)
    b.add("one_mismatch", mutate(g[100:150], subs={20}), 100, 150)
    b.add("three_mismatches", mutate(g[100:150], subs={10, 25, 40}), 100, 150)
    b.add("inserted", mutate(g[200:250], ins={25}), 200, 250)
    b.add("deleted", mutate(g[300:351], dele={25}), 300, 351)
    n = g[720:770].copy(); n[13] = 4
    b.add("an_N", n, 720, 770)
    n = mutate(g[720:770], dele={30}); n[13] = 4
    b.add("an_N_and_a_gap", n, 720, 770)
    b.add("one_by_one", g[900:901], 900, 901)
    b.add("one_by_one_mismatch", (g[900:901] + 1) % 4, 900, 901)
    b.add("one_by_two", g[900:901], 900, 902)
    b.add("two_by_one", g[900:902], 900, 901)
    J["simple"] = b.job()

    b = Builder()
    hp = mutate(g[480:530], dele={25})                 # one A less in the run g[500:510]
    hpi = np.concatenate([g[480:505], [0], g[505:530]]).astype(np.uint8)     # one A more
    for rev in (False, True):
        s = "_rev" if rev else "_fwd"
        b.add("homopolymer_del" + s, hp, 480, 530, rev=rev)
        b.add("homopolymer_ins" + s, hpi, 480, 530, rev=rev)
        rd = mutate(g[1000:1060], subs={30}, dele={40})
        full = np.concatenate([[3, 3, 3, 3, 3], rd, [2, 2, 2, 2, 2, 2, 2]]).astype(np.uint8)
        # clips: 5 bases in front of and 7 behind the aligned part (of the forward-sense read)
        qb, qe = (7, 7 + len(rd)) if rev else (5, 5 + len(rd))
        b.add("clips" + s, full, 1000, 1060, rev=rev, qb=qb, qe=qe)
        b.add("second_contig_start" + s, g[700:740], 700, 740, rev=rev)
        b.add("first_contig_end" + s, mutate(g[650:700], subs={3, 9, 44}), 650, 700, rev=rev)
    b.add("crosses_L", g[1550:1600], 1550, 1600, raw=dict(re=1650 - (1550 - 7)))
    b.add("all_minus_one", g[100:150], 100, 150, raw={f: -1 for f in R.RESULT_DTYPE.names})
    b.add("empty_query", g[100:150], 100, 150, raw=dict(qe=0))
    b.add("empty_text", g[100:150], 100, 150, raw=dict(re=7))
    J["strand"] = b.job()

    b = Builder()
    for rev in (False, True):
        s = "_rev" if rev else "_fwd"
        b.add("leading_deletion" + s, g[105:150], 100, 150, rev=rev, truesc=45)
        b.add("trailing_deletion" + s, g[100:145], 100, 150, rev=rev, truesc=45)
        b.add("both_ends" + s, g[105:145], 100, 150, rev=rev, truesc=40)
        b.add("leading_insertion" + s, np.concatenate([[1, 2, 3], g[100:150]]).astype(np.uint8), 100, 150, rev=rev, truesc=50)
        b.add("inner_and_leading" + s, mutate(g[105:160], dele={130}), 100, 160, rev=rev, truesc=40)
    J["squeeze"] = b.job()

    # ties: two letters, unit costs - m == e, h == f, e == t and f == t all come up (the CPU test checks that they do)
    rng = np.random.default_rng(5)
    g2 = genome()
    g2[1100:1400] = rng.integers(0, 2, 300)
    b = Builder(g=g2, a=1, b=1, o_del=1, e_del=1, o_ins=1, e_ins=1)
    for c in range(24):
        lt, lqq = int(rng.integers(6, 22)), int(rng.integers(6, 22))
        at = 1100 + int(rng.integers(0, 270))
        b.add("tie%d" % c, rng.integers(0, 2, lqq).astype(np.uint8), at, at + lt, rev=bool(c & 1), truesc=int(rng.integers(0, 12)), rw=int(rng.integers(0, 30)))
    J["ties"] = b.job()

    # tries
    b = Builder(w=4)
    far = np.concatenate([g[1100:1120], [1, 2, 3, 0, 1, 2, 3, 0], g[1120:1180], g[1188:1200]]).astype(np.uint8)   # 8 in, 8 out
    best = R.global_rolling([int(c) for c in far], [int(c) for c in g[1100:1200]], 103, R.params())[0]
    b.add("band_doubles_twice", far, 1100, 1200, truesc=best, rw=2)
    b.add("band_doubles_twice_rev", far, 1100, 1200, truesc=best, rw=2, rev=True)
    b.add("capped_by_the_results_w", far, 1100, 1200, truesc=best, rw=5)
    b.add("not_capped", far, 1100, 1200, truesc=best, rw=1000)
    b.add("same_score_stops", mutate(g[100:150], subs={10, 25, 40}), 100, 150, truesc=1000, rw=1)
    b.add("same_score_stops_dp", mutate(g[300:351], dele={25}), 300, 351, truesc=1000, rw=1)
    J["tries"] = b.job()
    b = Builder(w=1)
    b.add("stops_at_4w", far, 1100, 1200, truesc=best, rw=50)
    b.add("stops_at_4w_equal_lengths", mutate(g[100:150], subs={10, 25, 40}), 100, 150, truesc=1000, rw=50)
    J["tries_4w"] = b.job()
    b = Builder(w=0)
    b.add("w_zero", mutate(g[100:150], subs={10, 25, 40}), 100, 150, truesc=1000, rw=50)
    b.add("w_zero_gap", far, 1100, 1200, truesc=best, rw=50)
    J["tries_w0"] = b.job()

    # band: 2 w + 1 < |Q| with rows past w; strips: |Q| around the multiples of 64; a band wider than a strip
    b = Builder()
    b.add("narrow_band_60", mutate(g[800:860], subs={5, 30, 50}), 800, 860)
    for lqq in (63, 64, 65, 127, 128, 129):
        for kind, dl in (("ins", -1), ("del", 1), ("sub", 0)):
            subs = {7, lqq // 2, lqq - 5} | ({20, 41, 60} if lqq > 100 else set())
            rd = mutate(g[900:900 + lqq + dl], subs, ins={lqq - 9} if kind == "ins" else (), dele={lqq - 9} if kind == "del" else ())
            assert len(rd) == lqq
            b.add("q%d_%s" % (lqq, kind), rd, 900, 900 + lqq + dl, rev=(lqq & 1) == 0 and kind != "sub")
    b.add("band_wider_than_a_strip", mutate(g[1000:1130], subs={17, 70, 120}, dele=set(range(100, 103))), 990, 1200, truesc=100)
    b.add("band_wider_than_a_strip_rev", mutate(g[1000:1130], subs={17, 70, 120}, ins={90}), 990, 1200, truesc=100, rev=True)
    b.add("query_longer", np.concatenate([g[1000:1050], genome(3)[0:70], g[1050:1100]]).astype(np.uint8), 1000, 1100, truesc=70)
    J["band_and_strips"] = b.job()

    b = Builder(a=2, b=3, o_del=5, e_del=2, o_ins=4, e_ins=1)
    b.add("perfect", g[100:150], 100, 150)
    b.add("three_mismatches", mutate(g[100:150], subs={10, 25, 40}), 100, 150)
    b.add("two_deleted", mutate(g[300:352], dele={25, 26}), 300, 352, rev=True)
    b.add("three_inserted", np.concatenate([g[200:225], [1, 1, 2], g[225:250]]).astype(np.uint8), 200, 250)
    b.add("homopolymer_del", hp, 480, 530, rev=True)
    b.add("q129", mutate(g[900:1030], subs={7, 64, 120}, dele={100}), 900, 1030)
    J["scoring"] = b.job()
    return J


def synthetic(n, seed, read_len=(30, 140), **params):
    """n generated regions on both strands with substitutions, short indels and clips; some invalid results in between."""
    rng = np.random.default_rng(seed)
    g = genome(seed + 1, 4000)
    b = Builder(g=g, contig_off=[0, 1500, 4000], **params)
    for c in range(n):
        ln = int(rng.integers(read_len[0], read_len[1] + 1))
        at = int(rng.integers(0, len(g) - ln - 20))
        piece = g[at:at + ln]
        subs = set(int(x) for x in rng.integers(0, ln, int(rng.integers(0, 5))))
        ins = set(int(x) for x in rng.integers(2, ln - 2, int(rng.integers(0, 2))))
        dele = set(int(x) for x in rng.integers(2, ln - 2, int(rng.integers(0, 3))))
        rd = mutate(piece, subs, ins, dele)
        c5, c3 = (int(rng.integers(0, 6)) if rng.random() < 0.3 else 0 for _ in range(2))
        full = np.concatenate([rng.integers(0, 4, c5), rd, rng.integers(0, 4, c3)]).astype(np.uint8)
        rev = bool(rng.random() < 0.5)
        qb, qe = (c3, c3 + len(rd)) if rev else (c5, c5 + len(rd))
        a = b.p["mat"][0]
        truesc = len(rd) * a - 5 * len(subs) - 7 * (len(ins) + len(dele))
        raw = {f: -1 for f in R.RESULT_DTYPE.names} if c % 9 == 4 else None
        b.add("r%d" % c, full, at, at + ln, rev=rev, qb=qb, qe=qe, truesc=truesc, rw=int(rng.integers(0, 120)), raw=raw)
    return b.job()


def p_of(j):
    return R.params(**j["params"])


def reference(j, lookup=R.global_rolling):
    return R.run(p_of(j), j["seeds"], j["res"], j["text"], j["qer"], j["L"], j["contig_off"], lookup)


def reference_c(j):
    return R.run_c(p_of(j), j["seeds"], j["res"], j["text"], j["qer"], j["L"], j["contig_off"])


def same(got, want):
    ga, gc = got
    wa, wc = want
    assert ga.dtype == wa.dtype and len(ga) == len(wa)
    for f in wa.dtype.names:
        bad = np.nonzero(ga[f] != wa[f])[0]
        assert len(bad) == 0, "field %s differs at records %s: %s != %s" % (f, bad[:5], ga[f][bad[:5]], wa[f][bad[:5]])
    assert ga.tobytes() == wa.tobytes()
    assert len(gc) == len(wc) and np.array_equal(gc, wc), "CIGAR words differ"


def cigar_of(alns, cigar, k):
    o, n = int(alns[k]["cigar_off"]), int(alns[k]["n_cigar"])
    return "".join("%d%s" % (int(w) >> 4, "MIDNSHP=X"[int(w) & 15]) for w in cigar[o:o + n])


def check_invariants(j, alns, cigar):
    """What holds for every aligned record whatever bwa does: the CIGAR's query length is lq; its reference length plus the
    squeezed deletion is re - rb; the unclipped CIGAR rescored with mat and the gap costs gives `score`; nm recounted."""
    p = p_of(j)
    res = np.ascontiguousarray(j["res"]).view(R.RESULT_DTYPE).reshape(-1)
    L = j["L"]
    for k in range(len(alns)):
        a = alns[k]
        if a["rid"] < 0:
            assert a["n_cigar"] == 0
            continue
        s, r = j["seeds"][k], res[k]
        lq, qb, qe = int(s["lq"]), int(r["qb"]), int(r["qe"])
        rb, re = int(s["roff"]) + int(r["rb"]), int(s["roff"]) + int(r["re"])
        words = [(int(w) & 15, int(w) >> 4) for w in cigar[int(a["cigar_off"]):int(a["cigar_off"]) + int(a["n_cigar"])]]
        assert all(ln > 0 for _, ln in words) and all(x[0] != y[0] for x, y in zip(words, words[1:]))
        assert sum(ln for op, ln in words if op in (R.M, R.I, R.S)) == lq
        core = [w for w in words if w[0] != R.S]
        assert all(op == R.S for op, _ in words[:1] + words[-1:] if op not in (R.M, R.I, R.D)) and len(words) - len(core) <= 2
        ref_len = sum(ln for op, ln in core if op in (R.M, R.D))
        squeezed = (re - rb) - ref_len
        assert squeezed >= 0
        is_rev = int(a["is_rev"])
        assert is_rev == (1 if rb >= L else 0)
        read = [min(int(c), 4) for c in j["qer"][int(s["qoff"]):int(s["qoff"]) + lq]]
        Q, T = read[qb:qe], [min(int(c), 4) for c in j["text"][rb:re]]
        if is_rev:
            Q, T = Q[::-1], T[::-1]
        # where the squeezed deletion was: in front exactly when the position moved
        p0 = 2 * L - re if is_rev else rb
        pos = int(a["pos"]) + int(j["contig_off"][a["rid"]])
        lead = pos - p0
        assert lead in (0, squeezed) and j["contig_off"][a["rid"]] <= pos < j["contig_off"][a["rid"] + 1]
        full = ([(R.D, lead)] if lead else []) + core + ([(R.D, squeezed)] if squeezed and not lead else [])
        score, nm, x, y = 0, 0, 0, 0
        for n, (op, ln) in enumerate(full):
            if op == R.M:
                score += sum(p["mat"][T[y + d] * 5 + Q[x + d]] for d in range(ln))
                nm += sum(1 for d in range(ln) if Q[x + d] != T[y + d])
                x += ln; y += ln
            elif op == R.I:
                score -= p["o_ins"] + p["e_ins"] * ln
                nm += ln; x += ln
            else:
                score -= p["o_del"] + p["e_del"] * ln
                nm += ln if 0 < n < len(full) - 1 else 0
                y += ln
        assert x == len(Q) and y == len(T)
        assert score == a["score"], (k, score, int(a["score"]))
        assert nm == a["nm"], (k, nm, int(a["nm"]))
        assert 1 <= a["tries"] <= 3


def example():
    with open(os.path.join(HERE, "golden", "mem_cigar_example.json")) as f:
        return json.load(f)
