// mm_sam_rules.h — from "region g of an aligned batch" to its SAM record or its PAF line with cs:Z: / MD:Z: and = / X operations
// (DESIGN 3.21).  One text for the device (mm_sam_kernels.hip: a wavefront per line) and for a plain C++ build on the host
// (shims/mm_sam_cpu_twin.cpp, one lane), which the CPU tests hold against the restatement tests/mm_sam_ref.py.
// UPSTREAM-KNOWLEDGE: the rules follow minimap2's mm_write_sam3, write_cs_core, write_MD_core and mm_update_cigar_eqx as
// published; no compiled reference pins them.
//
// A function takes a team T: lane() of size() lanes (size() at most 64), sync(), ballot(b): bit l set iff lane l passed true,
// scan(v, &total): the sum of the v of the lanes below this one and, in every lane, the sum of all, shfl(v, l): lane l's v.
// Everything a function returns, and o.n, is the same in every lane.
//
// A line's length and its bytes come from one function over MmSamOut<WRITE>: the counting sink only adds, the storing sink
// also stores, below cap only.  Where every byte goes is a prefix sum of widths, so the bytes do not depend on scheduling.
// The alignment's columns are walked size() at a time: one load of each side a lane, a ballot of the unequal columns, and each
// lane the tokens that end at its column (`:n`, `*xy`, an = / X word, an MD count and letter), placed by a scan of their widths.
// A run of equal columns that leaves a step is carried in a team-uniform count, so no lane ever takes a trip per mismatch.
// Every loop is counted on entry: words, columns / size(), regions of a read, digits.
#pragma once
#include "mm_paf_rules.h"

namespace gbx {

struct MmSamSolo {
    int lane() const { return 0; }
    int size() const { return 1; }
    void sync() const {}
    uint64_t ballot(bool b) const { return b ? 1 : 0; }
    int64_t scan(int64_t v, int64_t *total) const { *total = v; return 0; }
    int64_t shfl(int64_t v, int) const { return v; }
};

template <bool WRITE>
struct MmSamOut {
    uint8_t *out; int64_t at, cap, n;                                     // the line starts at out[at]; n: its bytes so far
    GBX_MM_HD void put(int64_t i, uint8_t c) const { if (WRITE && at + i < cap) out[at + i] = c; }      // byte i of the line
};

struct MmSamView {                                 // the batch: what gbx_mm_sam_* takes
    MmPafView paf;
    const int64_t *reg_off;
    const uint8_t *seq, *qual, *tseq;              // qual null: QUAL prints `*`
    gbx_mm_sam_params P;
};

GBX_MM_HD inline uint64_t ms_below(int i) { return i >= 64 ? ~0ull : (1ull << i) - 1; }
GBX_MM_HD inline int ms_hibit(uint64_t m) { return 63 - __builtin_clzll(m); }
GBX_MM_HD inline int ms_digits(uint64_t a)
{
    int d = 1;
    for (uint64_t p = 10; d < 20 && a >= p; p *= 10) ++d;
    return d;
}
GBX_MM_HD inline uint8_t ms_digit(uint64_t a, int nd, int k)             // digit k from the left of a's nd
{
    for (int i = nd - 1 - k; i > 0; --i) a /= 10;
    return (uint8_t)('0' + a % 10);
}
// the columns of the step right before column i that are no breakers, with the carry where they reach the step's start
GBX_MM_HD inline int32_t ms_run_before(uint64_t brk, int i, int32_t carry)
{
    const uint64_t p = brk & ms_below(i);
    return p ? i - 1 - ms_hibit(p) : i + carry;
}
GBX_MM_HD inline uint8_t ms_comp(uint8_t c)
{
    const char *f = "ACGTUMRWSYKVHDBN", *t = "TGCAAKYWSRMBDHVN";
    const uint8_t u = c & 0xdf;
    for (int i = 0; i < 16; ++i)
        if ((uint8_t)f[i] == u) return (uint8_t)t[i] | (c & 0x20);
    return c;
}
GBX_MM_HD inline uint8_t ms_op_letter(uint32_t op) { return op < 9 ? (uint8_t)"MIDNSHP=X"[op] : (uint8_t)'?'; }

// ---- the team's writes: every lane calls them alike
template <bool W, class T>
GBX_MM_HD inline void ms_ch(const T &tm, MmSamOut<W> &o, uint8_t c)
{
    if (W && tm.lane() == 0) o.put(o.n, c);
    ++o.n;
}
template <bool W, class T>
GBX_MM_HD inline void ms_bytes(const T &tm, MmSamOut<W> &o, const uint8_t *s, int64_t len)
{
    if (len <= 0) return;
    if (W) for (int64_t i = tm.lane(); i < len; i += tm.size()) o.put(o.n + i, s[i]);
    o.n += len;
}
template <bool W, class T>
GBX_MM_HD inline void ms_str(const T &tm, MmSamOut<W> &o, const char *s)
{
    int64_t len = 0;
    while (s[len]) ++len;
    ms_bytes(tm, o, (const uint8_t *)s, len);
}
template <bool W, class T>
GBX_MM_HD inline void ms_num(const T &tm, MmSamOut<W> &o, int64_t v)       // a lane a digit
{
    const uint64_t a = v < 0 ? 0 - (uint64_t)v : (uint64_t)v;
    const int nd = ms_digits(a), neg = v < 0;
    if (W) {
        if (neg && tm.lane() == 0) o.put(o.n, '-');
        for (int k = tm.lane(); k < nd; k += tm.size()) o.put(o.n + neg + k, ms_digit(a, nd, k));
    }
    o.n += neg + nd;
}
// [from, from + len) of the oriented read, or of its qualities (mirrored, not complemented)
template <bool W, class T>
GBX_MM_HD inline void ms_read_bytes(const T &tm, MmSamOut<W> &o, const uint8_t *s, int32_t qlen, int rev, bool comp, int64_t from, int64_t len)
{
    if (len <= 0) return;
    if (W)
        for (int64_t i = tm.lane(); i < len; i += tm.size()) {
            const int64_t j = from + i;
            const uint8_t c = rev ? s[qlen - 1 - j] : s[j];
            o.put(o.n + i, rev && comp ? ms_comp(c) : c);
        }
    o.n += len;
}

template <bool W>
struct MsLane {                                    // one lane's token at byte p of the line
    const MmSamOut<W> &o; int64_t p;
    GBX_MM_HD void ch(uint8_t c) { o.put(p, c); ++p; }
    GBX_MM_HD void num(uint32_t v) { const int nd = ms_digits(v); for (int k = 0; k < nd; ++k) o.put(p + k, ms_digit(v, nd, k)); p += nd; }
};

// ---- an aligned region: its texts, its words and where they start (q0 in the oriented read)
struct MmSamAln { MmAlnSeq S; const uint32_t *cig; int32_t nw, t0, q0; };

// the clips of a record in the oriented read
GBX_MM_HD inline void ms_clips(const gbx_mm_aln &a, int rev, int32_t qlen, int32_t *c5, int32_t *c3)
{
    int64_t s = rev ? (int64_t)qlen - a.qe : a.qs, e = rev ? (int64_t)qlen - a.qs : a.qe;
    s = s < 0 ? 0 : s > qlen ? qlen : s;
    e = e < s ? s : e > qlen ? qlen : e;
    *c5 = (int32_t)s; *c3 = (int32_t)(qlen - e);
}

// The words with the columns they count: f(op, len, n, t, q), every lane alike, word after word; n the columns (bases of an I or
// D) the word counts, from column t of the contig and q of the oriented read.  A word counts at most to the end of the read
// (M, I) or of the contig (M, D), an op above 2 counts nothing.  size() words a trip while none is cut; a trip ends behind a
// word that is cut, so there are at most nw trips.
template <class T, class F>
GBX_MM_HD inline void ms_walk(const T &tm, const MmSamAln &A, F &f)
{
    int64_t t = A.t0, q = A.q0;
    const int32_t S = tm.size();
    for (int32_t k0 = 0, trips = 0; k0 < A.nw && trips < A.nw; ++trips) {
        const int32_t k = k0 + tm.lane(), left = A.nw - k0 < S ? A.nw - k0 : S;
        const uint32_t wd = k < A.nw ? A.cig[k] : 0;
        const int32_t op = (int32_t)(wd & 15);
        const int64_t len = wd >> 4, dt = op == 0 || op == 2 ? len : 0, dq = op == 0 || op == 1 ? len : 0;
        int64_t st, sq;
        const int64_t tp = t + tm.scan(dt, &st), qp = q + tm.scan(dq, &sq);
        const bool cut = tp + dt > A.S.tlen || qp + dq > A.S.qlen;
        const uint64_t cuts = tm.ballot(cut);
        int32_t take = cuts ? __builtin_ctzll(cuts) + 1 : left;
        if (take > left) take = left;
        int64_t n = op > 2 ? 0 : len;
        if (cut) {                                                     // only the first such lane is used: what lies before it is exact
            const int64_t rt = A.S.tlen - tp > 0 ? A.S.tlen - tp : 0, rq = A.S.qlen - qp > 0 ? A.S.qlen - qp : 0;
            if (op != 1 && n > rt) n = rt;
            if (op != 2 && n > rq) n = rq;
        }
        const int64_t ta = tp + (op == 0 || op == 2 ? n : 0), qa = qp + (op == 0 || op == 1 ? n : 0);
        for (int32_t kk = 0; kk < take; ++kk)
            f((int32_t)tm.shfl(op, kk), (int32_t)tm.shfl(len, kk), (int32_t)tm.shfl(n, kk), (int32_t)tm.shfl(tp, kk), (int32_t)tm.shfl(qp, kk));
        t = tm.shfl(ta, take - 1); q = tm.shfl(qa, take - 1);
        k0 += take;
    }
}

// one step of an M word: columns c0 .. of its n, a lane a column
struct MsStep { uint64_t neq; int32_t cnt; int tc, qc; bool valid, last; };
template <class T>
GBX_MM_HD inline MsStep ms_step(const T &tm, const MmAlnSeq &S, int32_t t, int32_t q, int32_t c0, int32_t n)
{
    MsStep s;
    const int32_t i = c0 + tm.lane();
    s.valid = i < n; s.last = i == n - 1;
    s.tc = s.valid ? S.tc(t + i) : 4; s.qc = s.valid ? S.qc(q + i) : 4;
    s.neq = tm.ballot(s.valid && s.tc != s.qc);
    s.cnt = n - c0 < tm.size() ? n - c0 : tm.size();
    return s;
}

// the letters of an I (the oriented read from q) or a D (the contig from t) out of tab[code]
template <bool W, class T>
GBX_MM_HD inline void ms_gap_letters(const T &tm, MmSamOut<W> &o, const MmAlnSeq &S, int32_t op, int32_t n, int32_t t, int32_t q, const char *tab)
{
    if (W) for (int32_t i = tm.lane(); i < n; i += tm.size()) o.put(o.n + i, (uint8_t)tab[op == 1 ? S.qc(q + i) : S.tc(t + i)]);
    o.n += n;
}

// ---- cs: form 1 short, 2 long
template <bool W, class T>
struct MsCs {
    const T &tm; MmSamOut<W> &o; const MmAlnSeq &S; int form;
    GBX_MM_HD void operator()(int32_t op, int32_t len, int32_t n, int32_t t, int32_t q)
    {
        (void)len;
        if (n <= 0) return;
        if (op != 0) { ms_ch(tm, o, op == 1 ? '+' : '-'); ms_gap_letters(tm, o, S, op, n, t, q, "acgtn"); return; }
        int32_t carry = 0;                                             // the equal columns that end the steps so far
        for (int32_t c0 = 0; c0 < n; c0 += tm.size()) {
            const MsStep s = ms_step(tm, S, t, q, c0, n);
            const int i = tm.lane();
            const bool ne = s.neq >> i & 1;
            int32_t w = 0, run = 0;
            if (s.valid) {
                const int32_t before = ms_run_before(s.neq, i, carry);
                if (form == 1) {
                    if (ne) { run = before; w = (run ? 1 + ms_digits(run) : 0) + 3; }
                    else if (s.last) { run = before + 1; w = 1 + ms_digits(run); }
                } else w = ne ? 3 : before == 0 ? 2 : 1;
            }
            int64_t total;
            const int64_t ex = tm.scan(w, &total);
            if (W && w) {
                MsLane<W> L{o, o.n + ex};
                if (run) { L.ch(':'); L.num(run); }
                if (ne) { L.ch('*'); L.ch("acgtn"[s.tc]); L.ch("acgtn"[s.qc]); }
                else if (form != 1) { if (w == 2) L.ch('='); L.ch("ACGTN"[s.qc]); }
            }
            o.n += total;
            carry = ms_run_before(s.neq, s.cnt, carry);
        }
    }
};

// ---- MD: the counter c runs on across words and I words
template <bool W, class T>
struct MsMd {
    const T &tm; MmSamOut<W> &o; const MmAlnSeq &S; int32_t c;
    GBX_MM_HD void operator()(int32_t op, int32_t len, int32_t n, int32_t t, int32_t q)
    {
        (void)len;
        if (n <= 0 || op == 1) return;
        if (op == 2) { ms_num(tm, o, c); ms_ch(tm, o, '^'); ms_gap_letters(tm, o, S, op, n, t, q, "ACGTN"); c = 0; return; }
        for (int32_t c0 = 0; c0 < n; c0 += tm.size()) {
            const MsStep s = ms_step(tm, S, t, q, c0, n);
            const int i = tm.lane();
            const bool ne = s.neq >> i & 1;
            const int32_t run = ne ? ms_run_before(s.neq, i, c) : 0, w = ne ? ms_digits(run) + 1 : 0;
            int64_t total;
            const int64_t ex = tm.scan(w, &total);
            if (W && w) { MsLane<W> L{o, o.n + ex}; L.num(run); L.ch("ACGTN"[s.tc]); }
            o.n += total;
            c = ms_run_before(s.neq, s.cnt, c);
        }
    }
    GBX_MM_HD void finish() { if (c > 0) ms_num(tm, o, c); }
};

// ---- the words with every M cut into = and X.  A run's word is written by the lane of the column behind it, the last run's by
// the lane of the word's last column as well.
template <bool W, class T>
struct MsEqx {
    const T &tm; MmSamOut<W> &o; const MmAlnSeq &S;
    GBX_MM_HD void operator()(int32_t op, int32_t len, int32_t n, int32_t t, int32_t q)
    {
        if (op != 0) { ms_num(tm, o, len); ms_ch(tm, o, ms_op_letter(op)); return; }
        int32_t carry = 0, carry_ne = 0;                               // the run that ends the steps so far, and whether it is unequal
        for (int32_t c0 = 0; c0 < n; c0 += tm.size()) {
            const MsStep s = ms_step(tm, S, t, q, c0, n);
            const uint64_t eqm = ~s.neq & ms_below(s.cnt);
            const int i = tm.lane();
            const int ne = (int)(s.neq >> i & 1);
            int32_t prev = 0, own = 0, w = 0;
            if (s.valid) {
                prev = ms_run_before(ne ? s.neq : eqm, i, carry_ne != ne ? carry : 0);      // the other kind's columns right before i
                if (s.last) own = ms_run_before(ne ? eqm : s.neq, i, carry_ne == ne ? carry : 0) + 1;
                w = (prev ? ms_digits(prev) + 1 : 0) + (own ? ms_digits(own) + 1 : 0);
            }
            int64_t total;
            const int64_t ex = tm.scan(w, &total);
            if (W && w) {
                MsLane<W> L{o, o.n + ex};
                if (prev) { L.num(prev); L.ch(ne ? '=' : 'X'); }
                if (own) { L.num(own); L.ch(ne ? 'X' : '='); }
            }
            o.n += total;
            const int e_ne = (int)(s.neq >> (s.cnt - 1) & 1);
            carry = ms_run_before(e_ne ? eqm : s.neq, s.cnt, carry_ne == e_ne ? carry : 0);
            carry_ne = e_ne;
        }
    }
};

// the words as they are, a lane a word
template <bool W, class T>
GBX_MM_HD inline void ms_cigar_plain(const T &tm, MmSamOut<W> &o, const uint32_t *cig, int32_t nw)
{
    for (int32_t k0 = 0; k0 < nw; k0 += tm.size()) {
        const int32_t k = k0 + tm.lane();
        const uint32_t wd = k < nw ? cig[k] : 0;
        const int32_t w = k < nw ? ms_digits(wd >> 4) + 1 : 0;
        int64_t total;
        const int64_t ex = tm.scan(w, &total);
        if (W && w) { MsLane<W> L{o, o.n + ex}; L.num(wd >> 4); L.ch(ms_op_letter(wd & 15)); }
        o.n += total;
    }
}
template <bool W, class T>
GBX_MM_HD inline void ms_cigar(const T &tm, MmSamOut<W> &o, const MmSamAln &A, int eqx)
{
    if (!eqx) { ms_cigar_plain(tm, o, A.cig, A.nw); return; }
    MsEqx<W, T> f{tm, o, A.S};
    ms_walk(tm, A, f);
}
template <bool W, class T>
GBX_MM_HD inline void ms_cs_md(const T &tm, MmSamOut<W> &o, const MmSamAln &A, const gbx_mm_sam_params &P)
{
    if (P.cs) { ms_str(tm, o, "\tcs:Z:"); MsCs<W, T> f{tm, o, A.S, P.cs}; ms_walk(tm, A, f); }
    if (P.md) { ms_str(tm, o, "\tMD:Z:"); MsMd<W, T> f{tm, o, A.S, 0}; ms_walk(tm, A, f); f.finish(); }
}

// ---- a region of the batch
struct MmSamReg {
    gbx_mm_reg reg; gbx_mm_aln a;
    bool aligned;                                  // it prints its alignment
    const uint8_t *qn, *tn; int64_t qnl, tnl; int32_t qlen, tlen;
    MmSamAln A;
};

// region g of read r (the read reg_off puts it in); false: it names another read and has no line
GBX_MM_HD inline bool ms_region(const MmSamView &V, int64_t g, int64_t r, MmSamReg *R)
{
    const MmPafView &F = V.paf;
    R->reg = F.regs[g];
    if (R->reg.read != r) return false;
    const gbx_mm_reg &reg = R->reg;
    const int64_t q0 = F.qname_off[r], q1 = F.qname_off[r + 1], s0 = F.seq_off[r], s1 = F.seq_off[r + 1];
    const bool tok = reg.rid >= 0 && reg.rid < F.n_targets;
    const int64_t n0 = tok ? F.tname_off[reg.rid] : 0, n1 = tok ? F.tname_off[reg.rid + 1] : 0;
    const int64_t t0 = tok ? F.tseq_off[reg.rid] : 0, t1 = tok ? F.tseq_off[reg.rid + 1] : 0;
    R->qn = F.qnames + q0; R->tn = tok ? F.tnames + n0 : nullptr;
    R->qnl = q1 > q0 ? q1 - q0 : 0; R->tnl = n1 > n0 ? n1 - n0 : 0;
    R->qlen = (int32_t)(s1 - s0); R->tlen = (int32_t)(t1 - t0);
    R->aligned = false;
    if (F.alns) {
        R->a = F.alns[g];
        const gbx_mm_aln &a = R->a;
        R->aligned = (a.flags & GBX_MM_ALN_ALIGNED) && !(a.flags & (GBX_MM_ALN_NO_ROOM | GBX_MM_ALN_INVALID)) && a.n_cigar >= 0 && a.cigar_off >= 0 &&
                     a.cigar_off + a.n_cigar <= F.cigar_cap;
    }
    if (R->aligned) {
        const int32_t ql = R->qlen > 0 ? R->qlen : 0, tl = R->tlen > 0 ? R->tlen : 0;
        int32_t c5, c3;
        ms_clips(R->a, reg.rev, ql, &c5, &c3);
        R->A.S = MmAlnSeq{V.tseq + t0, V.seq + s0, tl, ql, reg.rev ? 1 : 0};
        R->A.cig = F.cigar + R->a.cigar_off; R->A.nw = R->a.n_cigar;
        R->A.t0 = R->a.rs < 0 ? 0 : R->a.rs > tl ? tl : R->a.rs; R->A.q0 = c5;
    }
    return true;
}

// the regions of read r below n_regs, and which of them print an alignment
struct MmSamRead { int64_t g0, g1, primary; int32_t n_print, n_own; };      // n_own: printing regions with parent == id
template <class T>
GBX_MM_HD inline MmSamRead ms_read(const T &tm, const MmSamView &V, int64_t n_regs, int64_t r)
{
    MmSamRead D;
    int64_t g0 = V.reg_off[r], g1 = V.reg_off[r + 1];
    g0 = g0 < 0 ? 0 : g0 > n_regs ? n_regs : g0;
    g1 = g1 < g0 ? g0 : g1 > n_regs ? n_regs : g1;
    D.g0 = g0; D.g1 = g1; D.primary = -1; D.n_print = D.n_own = 0;
    for (int64_t b = g0; b < g1; b += tm.size()) {
        const int64_t g = b + tm.lane();
        MmSamReg R;
        const bool p = g < g1 && ms_region(V, g, r, &R) && R.aligned;
        const uint64_t bp = tm.ballot(p), bo = tm.ballot(p && R.reg.parent == R.reg.id);
        D.n_print += __builtin_popcountll(bp); D.n_own += __builtin_popcountll(bo);
        if (D.primary < 0 && bo) D.primary = b + __builtin_ctzll(bo);
    }
    return D;
}

// the tags NM .. rl of the `-c` PAF line
template <bool W, class T>
GBX_MM_HD inline void ms_tags(const T &tm, MmSamOut<W> &o, const gbx_mm_reg &g, const gbx_mm_aln &a, int32_t rep_len)
{
    ms_str(tm, o, "\tNM:i:"); ms_num(tm, o, a.nm); ms_str(tm, o, "\tms:i:"); ms_num(tm, o, a.dp_max); ms_str(tm, o, "\tAS:i:"); ms_num(tm, o, a.dp_score);
    ms_str(tm, o, "\tnn:i:"); ms_num(tm, o, a.n_ambi);
    ms_str(tm, o, g.parent == g.id ? "\ttp:A:P" : "\ttp:A:S");
    ms_str(tm, o, "\tcm:i:"); ms_num(tm, o, g.cnt);
    ms_str(tm, o, "\ts1:i:"); ms_num(tm, o, g.score);
    if (g.parent == g.id) { ms_str(tm, o, "\ts2:i:"); ms_num(tm, o, g.subsc); }
    ms_str(tm, o, "\trl:i:"); ms_num(tm, o, rep_len);
}

template <bool W, class T>
GBX_MM_HD inline void ms_paf_line(const T &tm, MmSamOut<W> &o, const MmSamView &V, const MmSamReg &R, int64_t r)
{
    const gbx_mm_reg &g = R.reg;
    const bool al = R.aligned;
    ms_bytes(tm, o, R.qn, R.qnl); ms_ch(tm, o, '\t'); ms_num(tm, o, R.qlen); ms_ch(tm, o, '\t'); ms_num(tm, o, al ? R.a.qs : g.qs); ms_ch(tm, o, '\t');
    ms_num(tm, o, al ? R.a.qe : g.qe); ms_ch(tm, o, '\t'); ms_ch(tm, o, g.rev ? '-' : '+'); ms_ch(tm, o, '\t');
    if (R.tn) ms_bytes(tm, o, R.tn, R.tnl); else ms_ch(tm, o, '*');
    ms_ch(tm, o, '\t'); ms_num(tm, o, R.tn ? R.tlen : 0); ms_ch(tm, o, '\t'); ms_num(tm, o, al ? R.a.rs : g.rs); ms_ch(tm, o, '\t');
    ms_num(tm, o, al ? R.a.re : g.re); ms_ch(tm, o, '\t'); ms_num(tm, o, al ? R.a.mlen : g.mlen); ms_ch(tm, o, '\t');
    ms_num(tm, o, al ? R.a.blen : g.blen); ms_ch(tm, o, '\t'); ms_num(tm, o, g.mapq);
    if (al) {
        ms_tags(tm, o, g, R.a, V.paf.rep_len[r]);
        ms_str(tm, o, "\tcg:Z:"); ms_cigar(tm, o, R.A, V.P.eqx);
        ms_cs_md(tm, o, R.A, V.P);
    } else {
        ms_str(tm, o, g.parent == g.id ? "\ttp:A:P" : "\ttp:A:S");
        ms_str(tm, o, "\tcm:i:"); ms_num(tm, o, g.cnt);
        ms_str(tm, o, "\ts1:i:"); ms_num(tm, o, g.score);
        if (g.parent == g.id) { ms_str(tm, o, "\ts2:i:"); ms_num(tm, o, g.subsc); }
        ms_str(tm, o, "\trl:i:"); ms_num(tm, o, V.paf.rep_len[r]);
    }
    ms_ch(tm, o, '\n');
}

// SEQ and QUAL of a SAM line: [from, from + len) of the oriented read; len < 0: `*` for both
template <bool W, class T>
GBX_MM_HD inline void ms_seq_qual(const T &tm, MmSamOut<W> &o, const MmSamView &V, int64_t r, int32_t qlen, int rev, int64_t from, int64_t len)
{
    const int64_t s0 = V.paf.seq_off[r];
    if (len < 0) { ms_str(tm, o, "*\t*"); return; }
    ms_read_bytes(tm, o, V.seq + s0, qlen, rev, true, from, len);
    ms_ch(tm, o, '\t');
    if (V.qual) ms_read_bytes(tm, o, V.qual + s0, qlen, rev, false, from, len); else ms_ch(tm, o, '*');
}

template <bool W, class T>
GBX_MM_HD inline void ms_sam_line(const T &tm, MmSamOut<W> &o, const MmSamView &V, const MmSamReg &R, const MmSamRead &D, int64_t g, int64_t r)
{
    const gbx_mm_reg &reg = R.reg;
    const gbx_mm_aln &a = R.a;
    const bool own = reg.parent == reg.id, secondary = !own, supp = own && g != D.primary;
    const int32_t qlen = R.A.S.qlen;
    int32_t c5, c3;
    ms_clips(a, reg.rev, qlen, &c5, &c3);
    const bool hard = (secondary || supp) && !V.P.softclip;
    ms_bytes(tm, o, R.qn, R.qnl); ms_ch(tm, o, '\t');
    ms_num(tm, o, (reg.rev ? 0x10 : 0) | (secondary ? 0x100 : 0) | (supp ? 0x800 : 0)); ms_ch(tm, o, '\t');
    if (R.tn) ms_bytes(tm, o, R.tn, R.tnl); else ms_ch(tm, o, '*');
    ms_ch(tm, o, '\t'); ms_num(tm, o, (int64_t)a.rs + 1); ms_ch(tm, o, '\t'); ms_num(tm, o, reg.mapq); ms_ch(tm, o, '\t');
    if (c5 > 0) { ms_num(tm, o, c5); ms_ch(tm, o, hard ? 'H' : 'S'); }
    ms_cigar(tm, o, R.A, V.P.eqx);
    if (c3 > 0) { ms_num(tm, o, c3); ms_ch(tm, o, hard ? 'H' : 'S'); }
    ms_str(tm, o, "\t*\t0\t0\t");
    if (secondary) ms_seq_qual(tm, o, V, r, qlen, reg.rev, 0, -1);
    else if (hard) ms_seq_qual(tm, o, V, r, qlen, reg.rev, c5, (int64_t)qlen - c5 - c3);
    else ms_seq_qual(tm, o, V, r, qlen, reg.rev, 0, qlen);
    ms_tags(tm, o, reg, a, V.paf.rep_len[r]);
    if (own && D.n_own >= 2) {
        ms_str(tm, o, "\tSA:Z:");
        for (int64_t h = D.g0; h < D.g1; ++h) {                        // the read's other printing records with parent == id
            if (h == g) continue;
            MmSamReg O;
            if (!ms_region(V, h, r, &O) || !O.aligned || O.reg.parent != O.reg.id) continue;
            int32_t o5, o3;
            ms_clips(O.a, O.reg.rev, qlen, &o5, &o3);
            const int64_t lq = (int64_t)O.a.qe - O.a.qs, lt = (int64_t)O.a.re - O.a.rs;
            if (O.tn) ms_bytes(tm, o, O.tn, O.tnl); else ms_ch(tm, o, '*');
            ms_ch(tm, o, ','); ms_num(tm, o, (int64_t)O.a.rs + 1); ms_ch(tm, o, ','); ms_ch(tm, o, O.reg.rev ? '-' : '+'); ms_ch(tm, o, ',');
            if (o5 > 0) { ms_num(tm, o, o5); ms_ch(tm, o, 'S'); }
            ms_num(tm, o, lq < lt ? lq : lt); ms_ch(tm, o, 'M');
            if (lq > lt) { ms_num(tm, o, lq - lt); ms_ch(tm, o, 'I'); }
            if (lt > lq) { ms_num(tm, o, lt - lq); ms_ch(tm, o, 'D'); }
            if (o3 > 0) { ms_num(tm, o, o3); ms_ch(tm, o, 'S'); }
            ms_ch(tm, o, ','); ms_num(tm, o, O.reg.mapq); ms_ch(tm, o, ','); ms_num(tm, o, O.a.nm); ms_ch(tm, o, ';');
        }
    }
    ms_cs_md(tm, o, R.A, V.P);
    ms_ch(tm, o, '\n');
}

// The line of region g of read r at out[at ..) below cap -> its length, in every lane; 0: the region prints nothing
template <bool W, class T>
GBX_MM_HD inline int64_t mm_sam_region_line(const T &tm, const MmSamView &V, int64_t n_regs, int64_t g, int64_t r, uint8_t *out, int64_t at, int64_t cap)
{
    MmSamOut<W> o{out, at, cap, 0};
    MmSamReg R;
    if (!ms_region(V, g, r, &R)) return 0;
    if (V.P.format == 0) { ms_paf_line(tm, o, V, R, r); return o.n; }
    if (!R.aligned) return 0;
    const MmSamRead D = ms_read(tm, V, n_regs, r);
    ms_sam_line(tm, o, V, R, D, g, r);
    return o.n;
}

// The line of read r when none of its regions prints (SAM format only) -> its length, else 0
template <bool W, class T>
GBX_MM_HD inline int64_t mm_sam_unmapped_line(const T &tm, const MmSamView &V, int64_t n_regs, int64_t r, uint8_t *out, int64_t at, int64_t cap)
{
    if (V.P.format == 0) return 0;
    const MmSamRead D = ms_read(tm, V, n_regs, r);
    if (D.n_print > 0) return 0;
    MmSamOut<W> o{out, at, cap, 0};
    const int64_t q0 = V.paf.qname_off[r], q1 = V.paf.qname_off[r + 1], ql = V.paf.seq_off[r + 1] - V.paf.seq_off[r];
    ms_bytes(tm, o, V.paf.qnames + q0, q1 - q0);
    ms_str(tm, o, "\t4\t*\t0\t0\t*\t*\t0\t0\t");
    ms_seq_qual(tm, o, V, r, (int32_t)ql, 0, 0, ql > 0 ? ql : 0);
    ms_ch(tm, o, '\n');
    return o.n;
}

// the host build: the text of every read in order -> its length; bytes below text_cap are written, line_off[n_reads + 1] and
// counts[2] (lines, regions that print nothing) always.  Every lane of the team calls it.
template <class T>
inline int64_t mm_sam_text(const T &tm, const MmSamView &V, int64_t n_regs, uint8_t *lines, int64_t text_cap, int64_t *line_off, int64_t *counts)
{
    int64_t at = 0, n_lines = 0, n_silent = 0;
    for (int64_t r = 0; r < V.paf.n_reads; ++r) {
        if (tm.lane() == 0) line_off[r] = at;
        const MmSamRead D = ms_read(tm, V, n_regs, r);
        for (int64_t g = D.g0; g < D.g1; ++g) {
            const int64_t n = mm_sam_region_line<true>(tm, V, n_regs, g, r, lines, at, text_cap);
            ++(n > 0 ? n_lines : n_silent);
            at += n;
        }
        const int64_t n = mm_sam_unmapped_line<true>(tm, V, n_regs, r, lines, at, text_cap);
        n_lines += n > 0;
        at += n;
    }
    if (tm.lane() == 0) { line_off[V.paf.n_reads] = at; counts[0] = n_lines; counts[1] = n_silent; }
    return at;
}

}  // namespace gbx
