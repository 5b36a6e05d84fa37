// mem_sam_kernels.hip — SAM records of the bwa-mem path (bwa's mem_aln2sam, add_cigar and the MD part of bwa_gen_cigar2): the
// regions of the regs / paired stage and the CIGAR stage's answer for their list -> one gbx_mem_sam_rec and one line of text per
// reported region, and one for a read with nothing reported.  The rules: DESIGN 3.15, include/gbx.h.
//   count    one read per wavefront: its reported regions -> the record offsets (mem_scan_launch)
//   records  one read per wavefront, lanes over its regions; the mate's reference length by the lanes over its CIGAR
//   measure  one record per wavefront: the MD walk and the line in counting mode -> md_len, line_len (mem_scan_launch over both)
//   write    one record per wavefront: the same walk and the same line with a sink that stores
// A line's length and its bytes come from one function, sam_line<WRITE>, and the MD string's from one, sam_md<WRITE>: the
// counting sink only advances.  Every call of a sink is made by the whole wavefront with uniform arguments.
#include "mem_common.h"

namespace gbx {
namespace {

struct SamAux {                      // what the later passes need of a record beyond gbx_mem_sam_rec (32 bytes)
    int32_t sel;                     // its gbx_mem_aln, -1: none
    int32_t msel;                    // the mate's, if the mate has a CIGAR, else -1
    int32_t rev;                     // the strand SEQ is printed on
    int32_t first, nlist;            // the read's records: wrec[first .. first + nlist)
    int32_t lq;
    int32_t hascig;                  // n_cigar > 0
    int32_t pad_;
};

struct SamArgs {
    MemSamIo io;
    int64_t n_reads; int mode, softclip;
    int64_t rec_max;
    gbx_mem_sam_rec *wrec; SamAux *aux;
    long long *cnt_rec;              // n_reads + 1
    long long *cnt_ml;               // 2 x (rec_max + 1): md_len, line_len -> md_off, line_off
};

__device__ inline bool sam_upstream_ok(const SamArgs &A) { const int64_t n = *A.io.n_regs; return n >= 0 && n <= A.io.reg_cap; }

// the read's regions [lo, hi), inside the regions there are
__device__ inline void sam_reg_range(const SamArgs &A, int64_t r, long long *lo, long long *hi)
{
    const long long n = *A.io.n_regs;
    long long a = A.io.reg_off[r], b = A.io.reg_off[r + 1];
    a = clampll(a, 0, n); b = clampll(b, a, n);
    *lo = a; *hi = b;
}

__device__ inline bool sam_reported(const SamArgs &A, const gbx_mem_reg &g) { return (g.flag & 1) && g.sel >= 0 && g.sel < A.io.n_alns; }

// the words of an alignment, none when they do not lie inside the words there are
__device__ inline int sam_words(const SamArgs &A, const gbx_mem_aln &a, const uint32_t **w)
{
    long long nc = *A.io.n_cigar;
    nc = nc < A.io.cigar_cap ? nc : A.io.cigar_cap;
    *w = A.io.cigar;
    if (a.n_cigar <= 0 || a.cigar_off < 0 || a.cigar_off > nc || a.n_cigar > nc - a.cigar_off) return 0;
    *w = A.io.cigar + a.cigar_off;
    return a.n_cigar;
}

__device__ inline int sam_op(uint32_t w) { const int op = (int)(w & 15u); return op <= 2 ? op : 4; }      // M I D, everything else a clip

__device__ inline int sam_read_len(const SamArgs &A, int64_t r, long long *off)
{
    const long long o = A.io.read_off[r];
    long long l = A.io.read_len[r];
    *off = 0;
    if (o < 0 || o >= A.io.qer_bytes || l <= 0) return 0;
    l = l < A.io.qer_bytes - o ? l : A.io.qer_bytes - o;
    *off = o;
    return (int)(l < (1ll << 30) ? l : (1ll << 30));
}

// ---- count
__global__ void __launch_bounds__(256) mem_sam_count_kernel(SamArgs A)
{
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= A.n_reads) return;
    long long n = 0;
    if (sam_upstream_ok(A)) {
        long long lo, hi;
        sam_reg_range(A, r, &lo, &hi);
        for (long long c = lo; c < hi; c += 64) {
            const bool rep = c + lane < hi && sam_reported(A, A.io.regs[c + lane]);
            n += __builtin_popcountll(__ballot(rep));
        }
        n = n ? n : 1;
    }
    if (lane == 0) A.cnt_rec[r] = n;
}

// ---- records
struct SamMate { int have, rid, rev, sel, hascig; long long pos, rlen; };

__device__ inline long long sam_ref_len_lane(const uint32_t *w, int n)
{
    long long s = 0;
    for (int k = 0; k < n; ++k) { const int op = sam_op(w[k]); if (op == 0 || op == 2) s += w[k] >> 4; }
    return s;
}

// one lane makes record `which` of read r from its region g (nullptr: the unmapped record)
__device__ inline void sam_build(const SamArgs &A, int64_t r, int which, const gbx_mem_reg *g, const SamMate &m, int fl, long long base, int nlist,
                                 int lq)
{
    if (base + which >= A.rec_max) return;
    gbx_mem_sam_rec R;
    SamAux X;
    memset(&R, 0, sizeof(R));
    memset(&X, 0, sizeof(X));
    R.read = (int32_t)r; R.which = which; R.rid = -1; R.pos = -1; R.mrid = -1; R.mpos = -1;
    X.sel = -1; X.msel = -1; X.first = (int32_t)base; X.lq = lq;
    X.nlist = (int32_t)(nlist < A.rec_max - base ? nlist : A.rec_max - base);
    bool mapped = false;
    long long rlen = 0;
    int rev = 0;
    R.flag = fl;
    R.sq_b = 0; R.sq_e = lq;
    if (g) {
        const gbx_mem_aln a = A.io.alns[g->sel];
        if (a.rid >= 0 && a.rid < A.io.n_contigs) {
            mapped = true;
            const uint32_t *w;
            const int nw = sam_words(A, a, &w);
            R.rid = a.rid; R.pos = a.pos; R.mapq = g->mapq; R.nm = a.nm; R.as_ = g->score; R.xs = g->sub > g->csub ? g->sub : g->csub;
            R.flag |= g->flag & 0x800;
            R.n_cigar = nw; R.cigar_off = nw ? a.cigar_off : 0;
            rev = a.is_rev != 0;
            X.sel = g->sel; X.hascig = nw > 0;
            rlen = sam_ref_len_lane(w, nw);
            if (!A.softclip && which > 0 && nw > 0) {             // the clips print as H: SEQ loses them
                int c0 = sam_op(w[0]) == 4 ? (int)(w[0] >> 4) : 0;
                int c1 = nw > 1 && sam_op(w[nw - 1]) == 4 ? (int)(w[nw - 1] >> 4) : 0;
                c0 = c0 < lq ? c0 : lq; c1 = c1 < lq - c0 ? c1 : lq - c0;
                R.sq_b = rev ? c1 : c0; R.sq_e = lq - (rev ? c0 : c1);
            }
        }
    }
    if (!mapped) {
        R.flag |= 0x4;
        if (m.have) { R.rid = m.rid; R.pos = m.pos; rev = m.rev; }
    }
    if (A.mode) {
        if (m.have) { R.mrid = m.rid; R.mpos = m.pos; if (m.rev) R.flag |= 0x20; }
        else {
            R.flag |= 0x8;
            if (mapped) { R.mrid = R.rid; R.mpos = R.pos; if (rev) R.flag |= 0x20; }
        }
        if (mapped && X.hascig && m.have && m.hascig && R.rid == m.rid) {
            const long long p0 = R.pos + (rev ? rlen - 1 : 0), p1 = m.pos + (m.rev ? m.rlen - 1 : 0);
            R.tlen = -(p0 - p1 + (p0 > p1 ? 1 : p0 < p1 ? -1 : 0));
        }
        if (m.have && m.hascig) X.msel = m.sel;
    }
    if (rev) R.flag |= 0x10;
    X.rev = rev;
    A.wrec[base + which] = R;
    A.aux[base + which] = X;
}

__global__ void __launch_bounds__(256) mem_sam_rec_kernel(SamArgs A)
{
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= A.n_reads || !sam_upstream_ok(A)) return;
    const long long base = A.cnt_rec[r];
    const int nlist = (int)(A.cnt_rec[r + 1] - base);
    long long qoff;
    const int lq = sam_read_len(A, r, &qoff);
    // the mate: the first record of the other end
    SamMate m = {0, -1, 0, -1, 0, -1, 0};
    int fl = 0;
    if (A.mode) {
        fl = 0x1 | (r & 1 ? 0x80 : 0x40) | (A.io.pairs[r >> 1].proper ? 0x2 : 0);
        long long lo, hi;
        sam_reg_range(A, r ^ 1, &lo, &hi);
        long long mg = -1;
        for (long long c = lo; c < hi; c += 64) {
            const unsigned long long b = __ballot(c + lane < hi && sam_reported(A, A.io.regs[c + lane]));
            if (b) { mg = c + __builtin_ctzll(b); break; }
        }
        if (mg >= 0) {
            const gbx_mem_aln a = A.io.alns[A.io.regs[mg].sel];
            if (a.rid >= 0 && a.rid < A.io.n_contigs) {
                const uint32_t *w;
                const int nw = sam_words(A, a, &w);
                long long s = 0;
                for (int k = lane; k < nw; k += 64) { const int op = sam_op(w[k]); if (op == 0 || op == 2) s += w[k] >> 4; }
                for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d);
                m.have = 1; m.rid = a.rid; m.rev = a.is_rev != 0; m.sel = A.io.regs[mg].sel; m.hascig = nw > 0; m.pos = a.pos; m.rlen = s;
            }
        }
    }
    long long lo, hi;
    sam_reg_range(A, r, &lo, &hi);
    int n_rep = 0;
    for (long long c = lo; c < hi; c += 64) {
        gbx_mem_reg g;
        const bool in = c + lane < hi;
        if (in) g = A.io.regs[c + lane];
        const bool rep = in && sam_reported(A, g);
        const unsigned long long b = __ballot(rep);
        if (rep) sam_build(A, r, n_rep + __builtin_popcountll(b & below), &g, m, fl, base, nlist, lq);
        n_rep += __builtin_popcountll(b);
    }
    if (n_rep == 0 && lane == 0) sam_build(A, r, 0, nullptr, m, fl, base, nlist, lq);     // nothing reported: the unmapped record
}

// ---- the sink: a position in a byte buffer; WRITE = false only advances.  A second buffer (the md bytes) can ride along
template <bool WRITE>
struct SamSink {
    uint8_t *d; long long cap, pos;
    uint8_t *d2; long long cap2, delta2;          // d2 != nullptr: byte pos also goes to d2[pos + delta2]
    int lane;

    __device__ inline void st(long long o, uint8_t c) const
    {
        if (!WRITE) return;
        if (o < cap) d[o] = c;
        if (d2 && o + delta2 < cap2) d2[o + delta2] = c;
    }
    __device__ inline void ch(char c) { if (WRITE && lane == 0) st(pos, (uint8_t)c); ++pos; }
    __device__ inline void lit(const char *s, int n) { if (WRITE && lane < n) st(pos + lane, (uint8_t)s[lane]); pos += n; }      // n <= 64
    __device__ inline void bytes(const uint8_t *s, long long n)
    {
        if (WRITE) for (long long k = lane; k < n; k += 64) st(pos + k, s[k]);
        pos += n;
    }
    static __device__ inline int digits(unsigned long long u)
    {
        int nd = 1;
        for (int k = 0; k < 19; ++k) { if (u < 10) break; u /= 10; ++nd; }
        return nd;
    }
    // lane k writes digit k of u at o
    static __device__ inline uint8_t digit(unsigned long long u, int nd, int k)
    {
        unsigned long long p = 1;
        for (int t = nd - 1 - k; t > 0; --t) p *= 10;
        return (uint8_t)('0' + (u / p) % 10);
    }
    __device__ inline void num(long long v)
    {
        unsigned long long u = (unsigned long long)v;
        if (v < 0) { ch('-'); u = 0ull - u; }
        const int nd = digits(u);
        if (WRITE && lane < nd) st(pos + lane, digit(u, nd, lane));
        pos += nd;
    }
    // CIGAR words as text, 64 words a step; s2h: every clip prints as H
    __device__ inline void cigar(const uint32_t *w, int n, bool s2h)
    {
        for (int c = 0; c < n; c += 64) {
            const bool in = c + lane < n;
            const uint32_t x = in ? w[c + lane] : 0;
            const int nd = digits(x >> 4);
            const int wd = in ? nd + 1 : 0;
            const int end = wave_scan_incl(wd, lane);
            if (WRITE && in) {
                const long long o = pos + end - wd;
                for (int k = 0; k < nd; ++k) st(o + k, digit(x >> 4, nd, k));
                const int op = sam_op(x);
                st(o + nd, (uint8_t)(op == 4 ? (s2h ? 'H' : 'S') : "MID"[op]));
            }
            pos += __shfl(end, 63);
        }
    }
};

__device__ inline int sam_code(uint8_t c) { return c > 4 ? 4 : c; }

struct SamRead { const uint8_t *q; const uint8_t *qual; int lq; int rev; };
// base i of the read as SEQ prints it before any hard clip
__device__ inline int sam_base(const SamRead &Q, long long i)
{
    if (i < 0 || i >= Q.lq) return 4;
    const int c = sam_code(Q.rev ? Q.q[Q.lq - 1 - i] : Q.q[i]);
    return Q.rev && c < 4 ? 3 - c : c;
}

// the MD string of a record: rule 6
template <bool WRITE>
__device__ inline void sam_md(const SamArgs &A, SamSink<WRITE> &S, const SamRead &Q, const uint32_t *w, int nw, int rid, long long pos, int unit)
{
    const uint8_t *text = A.io.text;
    const long long tend = A.io.contig_off[rid + 1] < A.io.text_bytes ? A.io.contig_off[rid + 1] : A.io.text_bytes;
    long long t = A.io.contig_off[rid] + pos, i = 0, run = 0;
    int first = -1, last = -1;                    // the first and the last op that is no clip
    for (int k = 0; k < nw; ++k) if (sam_op(w[k]) != 4) { if (first < 0) first = k; last = k; }
    for (int k = 0; k < nw; ++k) {
        const int op = sam_op(w[k]);
        long long l = w[k] >> 4;
        if (op == 2) {
            const long long room = tend > t ? tend - t : 0;
            l = l < room ? l : room;
            if (k != first && k != last) {
                S.num(run); S.ch('^');
                if (WRITE) for (long long j = S.lane; j < l; j += 64) S.st(S.pos + j, (uint8_t)"ACGTN"[sam_code(t + j >= 0 ? text[t + j] : 4)]);
                S.pos += l;
                run = 0;
            }
            t += l;
            continue;
        }
        const long long left = Q.lq > i ? Q.lq - i : 0;
        l = l < left ? l : left;
        if (op == 0) {
            GBX_GUARD(trips, l / 64 + 2);
            for (long long j0 = 0; j0 < l; j0 += 64) {
                if (GBX_GUARD_TRIP(trips, GBX_GK_MEM, 60, unit)) break;
                const long long j = j0 + S.lane;
                const bool in = j < l;
                const int rc = in ? sam_base(Q, i + j) : 4;
                const int tc = in && t + j >= 0 && t + j < tend ? sam_code(text[t + j]) : 4;
                unsigned long long b = __ballot(in && rc != tc);
                const int nmm = __builtin_popcountll(b);
                int done = 0;
                for (int x = 0; x < nmm; ++x) {
                    const int at = __builtin_ctzll(b);
                    b &= b - 1;
                    S.num(run + at - done);
                    S.ch("ACGTN"[__shfl(tc, at)]);
                    run = 0; done = at + 1;
                }
                const long long cn = l - j0 < 64 ? l - j0 : 64;
                run += cn - done;
            }
            t += l;
        }
        i += l;
    }
    S.num(run);
}

template <bool WRITE>
__device__ inline void sam_contig(const SamArgs &A, SamSink<WRITE> &S, int rid)
{
    long long a = A.io.cname_off[rid], b = A.io.cname_off[rid + 1];
    a = clampll(a, 0, A.io.cname_bytes); b = clampll(b, a, A.io.cname_bytes);
    S.bytes(A.io.cnames + a, b - a);
}

// the line of record `rec`: rule 7.  md_dst: where the md bytes go besides the line (WRITE only), md_off their offset
template <bool WRITE>
__device__ inline void sam_line(const SamArgs &A, SamSink<WRITE> &S, long long rec, const gbx_mem_sam_rec &R, const SamAux &X, long long md_off,
                                long long *md_len)
{
    const int64_t r = R.read;
    long long qoff;
    sam_read_len(A, r, &qoff);
    SamRead Q = {A.io.qer + qoff, A.io.qual ? A.io.qual + qoff : nullptr, X.lq, X.rev};
    const bool s2h = !A.softclip && R.which > 0;
    const uint32_t *w = A.io.cigar + R.cigar_off;
    {
        long long a = A.io.name_off[r], b = A.io.name_off[r + 1];
        a = clampll(a, 0, A.io.name_bytes); b = clampll(b, a, A.io.name_bytes);
        S.bytes(A.io.names + a, b - a);
    }
    S.ch('\t'); S.num(R.flag); S.ch('\t');
    if (R.rid >= 0) {
        sam_contig(A, S, R.rid); S.ch('\t'); S.num(R.pos + 1); S.ch('\t'); S.num(R.mapq); S.ch('\t');
        if (R.n_cigar > 0) S.cigar(w, R.n_cigar, s2h); else S.ch('*');
    } else
        S.lit("*\t0\t0\t*", 7);
    S.ch('\t');
    if (R.mrid >= 0) {
        if (R.mrid == R.rid) S.ch('='); else sam_contig(A, S, R.mrid);
        S.ch('\t'); S.num(R.mpos + 1); S.ch('\t'); S.num(R.tlen);
    } else
        S.lit("*\t0\t0", 5);
    S.ch('\t');
    {   // SEQ and QUAL: [sq_b, sq_e) of the stored read, mirrored on the reverse strand
        const long long n = R.sq_e - R.sq_b;
        if (n > 0) {
            if (WRITE) for (long long k = S.lane; k < n; k += 64) {
                const int c = sam_code(X.rev ? Q.q[R.sq_e - 1 - k] : Q.q[R.sq_b + k]);
                S.st(S.pos + k, (uint8_t)(X.rev ? "TGCAN" : "ACGTN")[c]);
            }
            S.pos += n;
        } else
            S.ch('*');
        S.ch('\t');
        if (n > 0 && Q.qual) {
            if (WRITE) for (long long k = S.lane; k < n; k += 64) S.st(S.pos + k, X.rev ? Q.qual[R.sq_e - 1 - k] : Q.qual[R.sq_b + k]);
            S.pos += n;
        } else
            S.ch('*');
    }
    *md_len = 0;
    if (X.hascig) {
        S.lit("\tNM:i:", 6); S.num(R.nm); S.lit("\tMD:Z:", 6);
        const long long at = S.pos;
        if (WRITE) { S.d2 = A.io.md; S.cap2 = A.io.md_cap; S.delta2 = md_off - at; }
        sam_md<WRITE>(A, S, Q, w, R.n_cigar, R.rid, R.pos, (int)rec);
        S.d2 = nullptr;
        *md_len = S.pos - at;
    }
    if (X.msel >= 0) {
        const gbx_mem_aln ma = A.io.alns[X.msel];
        const uint32_t *mw;
        const int nmw = sam_words(A, ma, &mw);
        S.lit("\tMC:Z:", 6); S.cigar(mw, nmw, s2h);
    }
    if (R.as_ >= 0) { S.lit("\tAS:i:", 6); S.num(R.as_); }
    if (R.xs >= 0) { S.lit("\tXS:i:", 6); S.num(R.xs); }
    if (R.n_sa > 0) {
        S.lit("\tSA:Z:", 6);
        for (int k = 0; k < X.nlist; ++k) {
            const long long o = X.first + k;
            if (o == rec) continue;
            const gbx_mem_sam_rec O = A.wrec[o];
            if (O.flag & 0x4) continue;
            sam_contig(A, S, O.rid); S.ch(','); S.num(O.pos + 1); S.ch(','); S.ch(A.aux[o].rev ? '-' : '+'); S.ch(',');
            S.cigar(A.io.cigar + O.cigar_off, O.n_cigar, false);
            S.ch(','); S.num(O.mapq); S.ch(','); S.num(O.nm); S.ch(';');
        }
    }
    S.ch('\n');
}

// SA entries of a record: the other records of its read that are mapped (0 for an unmapped record)
__device__ inline int sam_count_sa(const SamArgs &A, long long rec, const gbx_mem_sam_rec &R, const SamAux &X)
{
    if (R.flag & 0x4) return 0;
    int n = 0;
    for (int k = 0; k < X.nlist; ++k) if (X.first + k != rec && !(A.wrec[X.first + k].flag & 0x4)) ++n;
    return n;
}

__device__ inline long long sam_n_recs(const SamArgs &A)
{
    const long long n = A.cnt_rec[A.n_reads];
    return sam_upstream_ok(A) ? (n < A.rec_max ? n : A.rec_max) : 0;
}

// ---- measure
__global__ void __launch_bounds__(256) mem_sam_measure_kernel(SamArgs A)
{
    const int lane = threadIdx.x & 63;
    const long long n = sam_n_recs(A), step = (long long)gridDim.x * 4;
    for (long long rec = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); rec < n; rec += step) {
        gbx_mem_sam_rec R = A.wrec[rec];
        const SamAux X = A.aux[rec];
        R.n_sa = sam_count_sa(A, rec, R, X);
        SamSink<false> S = {nullptr, 0, 0, nullptr, 0, 0, lane};
        long long md_len;
        sam_line<false>(A, S, rec, R, X, 0, &md_len);
        if (lane == 0) {
            A.wrec[rec].n_sa = R.n_sa; A.wrec[rec].md_len = (int32_t)md_len; A.wrec[rec].line_len = (int32_t)S.pos;
            A.cnt_ml[rec] = md_len; A.cnt_ml[A.rec_max + 1 + rec] = S.pos;
        }
    }
}

// ---- write
__global__ void __launch_bounds__(256) mem_sam_write_kernel(SamArgs A)
{
    const int lane = threadIdx.x & 63;
    const long long n = sam_n_recs(A), step = (long long)gridDim.x * 4;
    for (long long rec = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); rec < n; rec += step) {
        gbx_mem_sam_rec R = A.wrec[rec];
        const SamAux X = A.aux[rec];
        R.md_off = A.cnt_ml[rec]; R.line_off = A.cnt_ml[A.rec_max + 1 + rec];
        SamSink<true> S = {A.io.lines, A.io.text_cap, R.line_off, nullptr, 0, 0, lane};
        long long md_len;
        sam_line<true>(A, S, rec, R, X, R.md_off, &md_len);
        if (lane == 0 && rec < A.io.rec_cap) A.io.recs[rec] = R;
    }
}

// after an overflow of the stage before: the outputs zeroed
__global__ void __launch_bounds__(256) mem_sam_zero_kernel(SamArgs A)
{
    if (sam_upstream_ok(A)) return;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x, step = (long long)gridDim.x * 256;
    int32_t *const rw = (int32_t *)A.io.recs;
    const long long nw = A.io.rec_cap * (long long)(sizeof(gbx_mem_sam_rec) / 4);
    for (long long k = t; k < nw; k += step) rw[k] = 0;
    for (long long k = t; k < A.io.md_cap; k += step) A.io.md[k] = 0;
    for (long long k = t; k < A.io.text_cap; k += step) A.io.lines[k] = 0;
}

struct MsLayout { size_t o_cnt, o_ml, o_bsum, o_rec, o_aux, total; int blocks_r, blocks_m; };
MsLayout ms_layout(int64_t n_reads, int64_t rec_max)
{
    MsLayout L;
    L.blocks_r = mem_scan_blocks(n_reads); L.blocks_m = mem_scan_blocks(rec_max);
    L.o_cnt = 0;
    L.o_ml = L.o_cnt + align256((size_t)(n_reads + 1) * 8);
    L.o_bsum = L.o_ml + align256(2 * (size_t)(rec_max + 1) * 8);
    L.o_rec = L.o_bsum + align256(2 * (size_t)(L.blocks_r > L.blocks_m ? L.blocks_r : L.blocks_m) * 8);
    L.o_aux = L.o_rec + align256((size_t)rec_max * sizeof(gbx_mem_sam_rec));
    L.total = L.o_aux + align256((size_t)rec_max * sizeof(SamAux));
    return L;
}

}  // namespace

int64_t mem_sam_rec_max(int64_t n_reads, int64_t reg_cap, int64_t n_alns)
{
    n_reads = n_reads < 0 ? 0 : n_reads; reg_cap = reg_cap < 0 ? 0 : reg_cap; n_alns = n_alns < 0 ? 0 : n_alns;
    return n_reads + (reg_cap < n_alns ? reg_cap : n_alns);
}

size_t mem_sam_workspace_bytes(int64_t n_reads, int64_t reg_cap, int64_t n_alns)
{
    return ms_layout(n_reads < 0 ? 0 : n_reads, mem_sam_rec_max(n_reads, reg_cap, n_alns)).total;
}

int mem_sam_launch(const gbx_mem_sam_params *p, int64_t n_reads, int mode, const MemSamIo &io, void *d_work, size_t work_bytes, hipStream_t s)
{
    if (n_reads >= (1ll << 31) - 1 || io.reg_cap >= (1ll << 31)) { set_error("mem sam: more than 2^31 - 2 reads or regions in one call"); return GBX_ERR_UNSUPPORTED; }
    const int64_t rec_max = mem_sam_rec_max(n_reads, io.reg_cap, io.n_alns);
    const MsLayout L = ms_layout(n_reads, rec_max);
    if (work_bytes < L.total) { set_error("mem sam: workspace too small"); return GBX_ERR_ARG; }
    char *wb = (char *)d_work;
    SamArgs A;
    A.io = io; A.n_reads = n_reads; A.mode = mode; A.softclip = p->softclip; A.rec_max = rec_max;
    A.cnt_rec = (long long *)(wb + L.o_cnt); A.cnt_ml = (long long *)(wb + L.o_ml);
    A.wrec = (gbx_mem_sam_rec *)(wb + L.o_rec); A.aux = (SamAux *)(wb + L.o_aux);
    long long *const bsum = (long long *)(wb + L.o_bsum);
    const MemScanGuard guard = {io.n_regs, 0, io.reg_cap};
    const unsigned read_blocks = (unsigned)((n_reads + 3) / 4);
    const unsigned rec_blocks = (unsigned)std::min<int64_t>((rec_max + 3) / 4, 8192);
    GBX_HIP(hipMemsetAsync(A.cnt_ml, 0, 2 * (size_t)(rec_max + 1) * 8, s));
    if (n_reads > 0) {
        Stage st("mem_sam_count", s);
        hipLaunchKernelGGL(mem_sam_count_kernel, dim3(read_blocks), dim3(256), 0, s, A);
    }
    {
        Stage st("mem_sam_scan", s);
        mem_scan_launch({A.cnt_rec, n_reads, 1, bsum, L.blocks_r, {io.n_recs, nullptr}, io.rec_off, {guard, {nullptr, 0, 0}}}, s);
    }
    if (n_reads > 0) {
        Stage st("mem_sam_rec", s);
        hipLaunchKernelGGL(mem_sam_rec_kernel, dim3(read_blocks), dim3(256), 0, s, A);
    }
    if (rec_max > 0) {
        Stage st("mem_sam_measure", s);
        hipLaunchKernelGGL(mem_sam_measure_kernel, dim3(rec_blocks), dim3(256), 0, s, A);
    }
    {
        Stage st("mem_sam_scan2", s);
        mem_scan_launch({A.cnt_ml, rec_max, 2, bsum, L.blocks_m, {io.n_md, io.n_text}, nullptr, {guard, {nullptr, 0, 0}}}, s);
    }
    if (rec_max > 0) {
        Stage st("mem_sam_write", s);
        hipLaunchKernelGGL(mem_sam_write_kernel, dim3(rec_blocks), dim3(256), 0, s, A);
    }
    {
        Stage st("mem_sam_zero", s);
        hipLaunchKernelGGL(mem_sam_zero_kernel, dim3(256), dim3(256), 0, s, A);
    }
    GBX_HIP(hipGetLastError());
    GBX_GUARD_CHECK("mem sam");
    return GBX_OK;
}

}  // namespace gbx
