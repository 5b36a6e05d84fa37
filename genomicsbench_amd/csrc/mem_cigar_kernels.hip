// mem_cigar_kernels.hip — CIGAR, edit distance and position of extended seeds (bwa-mem's mem_reg2aln, bwa_gen_cigar2 and
// ksw_global2) for gfx950 (MI355X).
//
// Semantics: include/gbx.h and DESIGN 3.11 (restated in tests/mem_cigar_ref.py, which pins them).
//
// Shape: one record per wavefront.  The banded global alignment runs in strips of 64 query columns, a column per lane,
// skewed: at step t lane l is on target row t - l, so the cell's left neighbour (the horizontal f and the h that becomes the
// next row's diagonal) is what lane l - 1 made one step earlier and comes over with __shfl_up, together with the text base
// of the row.  H's diagonal, E and f stay in registers; the three tries run inside the kernel and only the score decides.
//   * strip edge: lane 63 leaves (h, f) per row in the record's room (two buffers, by strip parity); the next strip's lane 0
//     takes them, and the text bases, 64 rows at a time - one coalesced load per 64 steps, handed out with v_readlane.
//   * direction bytes: in global memory, in the skewed order they are made in - strip, step, lane - four steps packed to a
//     dword per lane, so a store is 256 contiguous bytes per wave every four steps, never a scattered byte.  One layout and
//     one code path for a 151-base read and an 8 k-base region; the room per record is what its widest band can need
//     (cg_need), handed out in index order by a scan, so the output does not depend on the scheduling.
//   * traceback: the walk reads that room.  Along an M run the next 64 cells of the diagonal are one load per lane and a
//     ballot finds the run's end, so the serial part is one trip per run or gap base, not per base.  It runs twice: once
//     to count the ops and the edit distance (align kernel), once to write the words at their final places (pack kernel),
//     with a scan of the counts in between - count, scan, pack as in mem_chain_kernels.hip.
//   * every loop is counted: tries, strips, steps; the walk ends after |Q| + |T| bases at the latest.
#include <algorithm>
#include "mem_common.h"

namespace gbx {
namespace {

constexpr int CG_INF = -0x40000000;
constexpr int CG_MAXLEN = 0x3fffffff;

static_assert(sizeof(gbx_mem_aln) == 48 && sizeof(gbx_mem_cigar_params) == 120, "records");

struct CgRec {                        // one record's region, from the seed and the extension's result
    long long qoff, rb, re;           // the read's start in qer; text coordinates
    int lq, qb, qe, truesc, rw;
    int lQ, lT;                       // qe - qb, re - rb
    int valid;                        // 1 aligned, 0 rid = -1, -1 a range outside its arena (rid = -1 too)
    int is_rev;
};

__host__ __device__ inline CgRec cg_record(const gbx_bsw_seed &s, const gbx_bsw_seed_result &r, long long text_bytes,
                                           long long qer_bytes, long long L)
{
    CgRec R;
    R.qoff = s.qoff; R.lq = s.lq; R.qb = r.qb; R.qe = r.qe; R.truesc = r.truesc; R.rw = r.w;
    R.rb = s.roff + r.rb; R.re = s.roff + r.re;
    R.lQ = R.qe - R.qb;
    const long long lt = R.re - R.rb;
    R.lT = lt > CG_MAXLEN ? CG_MAXLEN : (int)lt;
    R.is_rev = R.rb >= L;
    R.valid = 1;
    if (r.qb < 0 || R.qe <= R.qb || R.rb >= R.re || (R.rb < L && L < R.re)) R.valid = 0;
    else {
        const long long tend = text_bytes < 2 * L ? text_bytes : 2 * L;
        if (s.lq < 0 || s.qoff < 0 || s.qoff + s.lq > qer_bytes || R.qe > s.lq || R.rb < 0 || R.re > tend || lt >= CG_MAXLEN) R.valid = -1;
    }
    return R;
}

__host__ __device__ inline int cg_infer_bw(int l1, int l2, int score, int a, int q, int e)
{
    if (l1 == l2 && l1 * a - score < (q + e - a) * 2) return 0;
    const int w = (int)((double)((l1 < l2 ? l1 : l2) * a - score - q) / e + 2.);
    const int d = l1 < l2 ? l2 - l1 : l1 - l2;
    return w > d ? w : d;
}

__host__ __device__ inline int cg_first_band(const gbx_mem_cigar_params &p, const CgRec &R)
{
    const int a = p.mat[0];
    const int wd = cg_infer_bw(R.lQ, R.lT, R.truesc, a, p.o_del, p.e_del), wi = cg_infer_bw(R.lQ, R.lT, R.truesc, a, p.o_ins, p.e_ins);
    int w2 = wd > wi ? wd : wi;
    if (w2 > p.w) w2 = w2 < R.rw ? w2 : R.rw;
    return w2;
}

// the band ksw_global2 gets from bwa_gen_cigar2 for the try's band w_
__host__ __device__ inline int cg_band(const gbx_mem_cigar_params &p, int lQ, int lT, int w_)
{
    const int a = p.mat[0];
    const int max_ins = (int)((double)(((lQ + 1) >> 1) * a - p.o_ins) / p.e_ins + 1.);
    const int max_del = (int)((double)(((lQ + 1) >> 1) * a - p.o_del) / p.e_del + 1.);
    int g = max_ins > max_del ? max_ins : max_del;
    g = g > 1 ? g : 1;
    const int d = lT > lQ ? lT - lQ : lQ - lT;
    int wb = (int)(((long long)g + d + 1) >> 1);
    wb = wb < w_ ? wb : w_;
    wb = wb > d + 3 ? wb : d + 3;
    return wb;
}

// the room of one alignment: two strip-edge buffers of (h, f) per row, then per strip of 64 columns its steps' direction dwords
struct CgRoom { long long bnd_bytes, strip_bytes; int strips; };
__host__ __device__ inline CgRoom cg_room(int lQ, int lT, int wb)
{
    CgRoom M;
    M.strips = (lQ + 63) >> 6;
    const long long band_rows = 2ll * wb + 64, rows = lT < band_rows ? lT : band_rows;
    M.strip_bytes = ((rows + 63 + 3) >> 2) * 256;
    M.bnd_bytes = (8ll * lT + 255) & ~255ll;
    return M;
}
__host__ __device__ inline long long cg_room_bytes(const CgRoom &M) { return 2 * M.bnd_bytes + M.strips * M.strip_bytes; }

// what the record's widest try can need (0: every try is the one M run without a DP)
__host__ __device__ inline long long cg_need(const gbx_mem_cigar_params &p, const CgRec &R)
{
    const int w0 = cg_first_band(p, R);
    if (R.lQ == R.lT && (w0 == 0 || (p.w == 0 && w0 >= 0))) return 0;
    const long long w4 = 4ll * w0 < 4ll * p.w ? 4ll * w0 : 4ll * p.w;
    const int wmax = w0 < 0 ? w0 : (int)w4;
    return cg_room_bytes(cg_room(R.lQ, R.lT, cg_band(p, R.lQ, R.lT, wmax)));
}

struct CgSt { int n_core, squeeze, nodp, pad_; };   // align -> pack: ops before the squeeze; 1 leading / 2 trailing D removed

struct CgArgs {
    gbx_mem_cigar_params p;
    MemCigarIo io;
    long long n, z_bytes;
    long long *off;                  // [2][n + 1]: direction room / CIGAR words per record, then their exclusive scans
    CgSt *st;                        // [n]
    unsigned char *z;                // [z_bytes]
};

__device__ inline int cg_code(unsigned c) { return c > 4 ? 4 : (int)c; }

struct CgSeq {                       // the region's query and text, both reversed on the reverse strand
    const uint8_t *q, *t;
    int lQ, lT, rev;
    __device__ int Q(int j) const { return cg_code(q[rev ? lQ - 1 - j : j]); }
    __device__ int T(int i) const { return cg_code(t[rev ? lT - 1 - i : i]); }
};

__device__ inline CgRec cg_load(const CgArgs &A, long long k)
{
    return cg_record(A.io.seeds[k], A.io.res[k], A.io.text_bytes, A.io.qer_bytes, A.io.l_pac);
}

__device__ inline int cg_wave_sum(int v)
{
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// ---- the direction room every record asks for
__global__ void __launch_bounds__(256) mem_cigar_need_kernel(CgArgs A)
{
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= A.n) return;
    const CgRec R = cg_load(A, k);
    A.off[k] = R.valid == 1 ? cg_need(A.p, R) : 0;
}

// ---- ksw_global2 over the record's room: the score; the direction bytes stay behind for the walk
__device__ int cg_global(const gbx_mem_cigar_params &p, const CgSeq &S, int wb, const CgRoom &M, unsigned char *room, const int *smat, int lane)
{
    const int lQ = S.lQ, lT = S.lT;
    const int o_del = p.o_del, e_del = p.e_del, o_ins = p.o_ins, e_ins = p.e_ins, oe_del = o_del + e_del, oe_ins = o_ins + e_ins;
    int2 *const bnd0 = (int2 *)room, *const bnd1 = (int2 *)(room + M.bnd_bytes);
    unsigned *const zroom = (unsigned *)(room + 2 * M.bnd_bytes);
    const long long strip_dw = M.strip_bytes >> 2;
    int fin = 0;
    for (int s = 0; s < M.strips; ++s) {
        const int j0 = s << 6, j = j0 + lane;
        const int jl = j0 + 63 < lQ - 1 ? j0 + 63 : lQ - 1;
        const int t_lo = j0 > wb ? j0 - wb : 0;
        const long long ih = (long long)jl + wb;
        const int i_hi = ih < lT - 1 ? (int)ih : lT - 1;
        const int t_hi = i_hi + (jl - j0);
        const int2 *const br = (s & 1) ? bnd0 : bnd1;           // what strip s - 1 left
        int2 *const bw = (s & 1) ? bnd1 : bnd0;
        const bool edge = s + 1 < M.strips;
        const bool col = j < lQ;
        const int qc = col ? S.Q(j) : 4;
        const int sc0 = smat[qc], sc1 = smat[5 + qc], sc2 = smat[10 + qc], sc3 = smat[15 + qc], sc4 = smat[20 + qc];
        const int H0j = j == 0 ? 0 : -(o_ins + e_ins * j);
        int E = CG_INF, diag = CG_INF, hout = CG_INF, fout = CG_INF, tcur = 4;
        if (s > 0 && t_lo > 0 && lane == 0) diag = br[t_lo - 1].x;
        unsigned *const zs = zroom + s * strip_dw;
        unsigned zacc = 0;
        for (int tb = t_lo; tb <= t_hi; tb += 64) {
            // the next 64 rows' text bases and left-edge cells, a row per lane
            const int ir = tb + lane;
            const bool rowok = ir < lT;
            const int tch = rowok ? S.T(ir) : 4;
            int bh = CG_INF, bf = CG_INF;
            if (s > 0 && rowok) { const int2 v = br[ir]; bh = v.x; bf = v.y; }
            const int un = t_hi - tb + 1 < 64 ? t_hi - tb + 1 : 64;
            for (int u = 0; u < un; ++u) {
                const int t = tb + u;
                int hl = __shfl_up(hout, 1), fl = __shfl_up(fout, 1), tl = __shfl_up(tcur, 1);
                const int t0 = __builtin_amdgcn_readlane(tch, u), h0 = __builtin_amdgcn_readlane(bh, u), f0 = __builtin_amdgcn_readlane(bf, u);
                if (lane == 0) { hl = h0; fl = f0; tl = t0; }
                tcur = tl;
                const int i = t - lane;
                const bool act = col && i >= 0 && i < lT && j - i <= wb && i - j <= wb;
                unsigned d = 0;
                if (act) {
                    const int dg = i == 0 ? H0j : (j == 0 ? -(o_del + e_del * i) : diag);
                    const int beg = i > wb ? i - wb : 0;
                    const int f = j == beg ? CG_INF : fl;
                    const int sc = tcur == 0 ? sc0 : tcur == 1 ? sc1 : tcur == 2 ? sc2 : tcur == 3 ? sc3 : sc4;
                    const int m = dg + sc;
                    int e = E;
                    d = m >= e ? 0 : 1;
                    int h = m >= e ? m : e;
                    d = h >= f ? d : 2;
                    h = h >= f ? h : f;
                    const int t1 = m - oe_del;
                    e -= e_del;
                    d |= e > t1 ? 1u << 2 : 0;
                    E = e > t1 ? e : t1;
                    const int t2 = m - oe_ins, f2 = f - e_ins;
                    d |= f2 > t2 ? 2u << 4 : 0;
                    fout = f2 > t2 ? f2 : t2;
                    hout = h;
                    if (i == lT - 1 && j == lQ - 1) fin = h;
                    if (lane == 63 && edge) bw[i] = make_int2(hout, fout);
                }
                diag = hl;
                zacc |= d << ((u & 3) * 8);
                if ((u & 3) == 3 || u == un - 1) {
                    zs[(long long)((t - t_lo) >> 2) * 64 + lane] = zacc;
                    zacc = 0;
                }
            }
        }
        __syncthreads();                                         // (one wave: orders the edge stores before the next strip's loads)
    }
    return __shfl(fin, (lQ - 1) & 63);
}

// ---- the traceback.  sink(op, len, r) gets the merged ops last to first (r = 0: the last op of the CIGAR); -> their number.
// Every lane runs it with the same values.
template <class Sink>
__device__ inline int cg_walk(const CgSeq &S, int wb, const CgRoom &M, const unsigned char *room, int lane, long long unit, int *mismatches, Sink sink)
{
    const int lQ = S.lQ, lT = S.lT;
    const unsigned char *const zb = room + 2 * M.bnd_bytes;
    const int cap = (int)(M.strip_bytes >> 6);                   // steps a strip has room for
    auto zat = [&](int i, int k) -> unsigned {
        const int s = k >> 6, l = k & 63, j0 = s << 6;
        const int t_lo = j0 > wb ? j0 - wb : 0;
        const int tt = i + l - t_lo;
        if (tt < 0 || tt >= cap || s >= M.strips) return 0;
        return zb[s * M.strip_bytes + (long long)(tt >> 2) * 256 + l * 4 + (tt & 3)];
    };
    int i = lT - 1;
    const long long ke = (long long)i + wb + 1 < lQ ? (long long)i + wb + 1 : lQ;
    int k = (int)ke - 1;
    int which = 0, op = -1, len = 0, r = 0, mm = 0;
    auto push = [&](int o, int n) {
        if (o == op) { len += n; return; }
        if (op >= 0) { sink(op, len, r); ++r; }
        op = o; len = n;
    };
    GBX_GUARD(guard, (long long)lQ + lT + 2);
    for (long long left = (long long)lQ + lT; left > 0 && i >= 0 && k >= 0;) {      // every trip takes at least one base
        if (GBX_GUARD_TRIP(guard, GBX_GK_MEM, 20, unit)) break;
        if (which == 0) {
            // an M run: the next 64 cells down the diagonal, one per lane
            const int ii = i - lane, kk = k - lane;
            const bool in = ii >= 0 && kk >= 0;
            const bool is_m = in && (zat(ii, kk) & 3) == 0;
            const unsigned long long stop = __ballot(!is_m);
            const int run = stop ? __builtin_ctzll(stop) : 64;
            if (run > 0) {
                const bool x = lane < run && S.Q(kk) != S.T(ii);
                mm += __builtin_popcountll(__ballot(x));
                push(0, run);
                i -= run; k -= run; left -= run;
                continue;
            }
        }
        which = (zat(i, k) >> (which << 1)) & 3;
        if (which == 0) { mm += S.Q(k) != S.T(i); push(0, 1); --i; --k; }
        else if (which == 1) { push(2, 1); --i; }
        else { push(1, 1); --k; }
        --left;
    }
    if (i >= 0) push(2, i + 1);
    if (k >= 0) push(1, k + 1);
    if (op >= 0) { sink(op, len, r); ++r; }
    *mismatches = mm;
    return r;
}

// the record's room and its size; -1: it ends past z_bytes (a record that needs none always fits)
__device__ inline unsigned char *cg_room_of(const CgArgs &A, long long k, long long *have)
{
    const long long o = A.off[k], e = A.off[k + 1];
    *have = e == o ? 0 : e <= A.z_bytes ? e - o : -1;
    return A.z + o;
}

// ---- tries, alignment and the first walk of one record: everything of gbx_mem_aln but cigar_off, and the word count
__global__ void __launch_bounds__(64) mem_cigar_align_kernel(CgArgs A)
{
    __shared__ int smat[25];
    const long long k = blockIdx.x;
    const int lane = threadIdx.x;
    if (lane < 25) smat[lane] = A.p.mat[lane];
    __syncthreads();
    const gbx_mem_cigar_params &p = A.p;
    const CgRec R = cg_load(A, k);
    long long *const cnt = A.off + (A.n + 1);
    gbx_mem_aln o;
    o.pos = 0; o.cigar_off = 0; o.rid = -1; o.is_rev = 0; o.n_cigar = 0; o.nm = 0; o.score = 0; o.w = 0; o.tries = 0; o.pad_ = 0;
    CgSt st = {0, 0, 0, 0};
    long long have = 0;
    unsigned char *const room = cg_room_of(A, k, &have);
    if (R.valid == 1 && have < 0) o.rid = -2;
    if (R.valid != 1 || have < 0) {
        if (lane == 0) { A.io.alns[k] = o; A.st[k] = st; cnt[k] = 0; }
        return;
    }
    CgSeq S;
    S.q = A.io.qer + R.qoff + R.qb; S.t = A.io.text + R.rb; S.lQ = R.lQ; S.lT = R.lT; S.rev = R.is_rev;
    const int a = p.mat[0];
    const int w4 = 4 * p.w;                                      // (w is at most 2^27: the entries check it)
    int w2 = cg_first_band(p, R), last = -(1 << 30), score = 0, tries = 0, wl = 0, wb = 0, nodp = 0, mm = 0;
    for (int it = 0; it < 3; ++it) {
        w2 = w2 < w4 ? w2 : w4;
        if (R.lQ == R.lT && w2 == 0) {
            int sum = 0, x = 0;
            for (int j = lane; j < R.lQ; j += 64) {
                const int q = S.Q(j), t = S.T(j);
                sum += smat[t * 5 + q];
                x += q != t;
            }
            score = cg_wave_sum(sum); mm = cg_wave_sum(x); nodp = 1;
        } else {
            wb = cg_band(p, R.lQ, R.lT, w2);
            if (cg_room_bytes(cg_room(R.lQ, R.lT, wb)) > have) { have = -1; break; }      // (cg_need covers every try: not reached)
            score = cg_global(p, S, wb, cg_room(R.lQ, R.lT, wb), room, smat, lane);
            nodp = 0;
        }
        wl = w2; ++tries;
        if (score == last || w2 == w4) break;
        last = score;
        w2 *= 2;
        if (!(it + 1 < 3 && score < R.truesc - a)) break;
    }
    if (have < 0) {
        o.rid = -2;
        if (lane == 0) { A.io.alns[k] = o; A.st[k] = st; cnt[k] = 0; }
        return;
    }
    // the ops: their number, the gap bases the edit distance counts, a D at either end
    int n_core = 1, gaps = 0, lead_d = 0, trail_d = 0;
    if (!nodp) {
        int e_op = -1, e_len = 0, l_op = -1, l_len = 0;
        n_core = cg_walk(S, wb, cg_room(R.lQ, R.lT, wb), room, lane, k, &mm, [&](int op, int len, int r) {
            if (r == 0) { e_op = op; e_len = len; }
            if (op == 1 || (op == 2 && r > 0)) gaps += len;
            l_op = op; l_len = len;
        });
        if (l_op == 2 && n_core > 1) gaps -= l_len;
        lead_d = l_op == 2 ? l_len : 0;
        trail_d = e_op == 2 ? e_len : 0;
    }
    st.n_core = n_core; st.nodp = nodp;
    st.squeeze = lead_d > 0 ? 1 : trail_d > 0 ? 2 : 0;
    const long long L = A.io.l_pac;
    long long pp = R.is_rev ? 2 * L - R.re : R.rb;
    pp += lead_d;
    int lo = 0, hi = A.io.n_contigs + 1;                        // the first entry above pp
    for (int it = 0; it < 32; ++it) {
        if (lo >= hi) break;
        const int mid = (lo + hi) >> 1;
        if (A.io.contig_off[mid] <= pp) lo = mid + 1; else hi = mid;
    }
    int c = lo - 1;
    c = c < 0 ? 0 : c >= A.io.n_contigs ? A.io.n_contigs - 1 : c;
    const int clip5 = R.is_rev ? R.lq - R.qe : R.qb, clip3 = R.is_rev ? R.qb : R.lq - R.qe;
    o.rid = c; o.pos = pp - A.io.contig_off[c]; o.is_rev = R.is_rev;
    o.n_cigar = n_core - (st.squeeze ? 1 : 0) + (clip5 > 0) + (clip3 > 0);
    o.nm = mm + gaps; o.score = score; o.w = wl; o.tries = tries;
    if (lane == 0) { A.io.alns[k] = o; A.st[k] = st; cnt[k] = o.n_cigar; }
}

// ---- cigar_off of every record, and the words at their final places (the walk again, now with somewhere to write)
__global__ void __launch_bounds__(64) mem_cigar_pack_kernel(CgArgs A)
{
    const long long k = blockIdx.x;
    const int lane = threadIdx.x;
    const long long base = A.off[A.n + 1 + k];
    if (lane == 0) A.io.alns[k].cigar_off = base;
    const int n_cigar = A.io.alns[k].n_cigar;
    if (n_cigar <= 0) return;
    const CgRec R = cg_load(A, k);
    const CgSt st = A.st[k];
    const int clip5 = R.is_rev ? R.lq - R.qe : R.qb, clip3 = R.is_rev ? R.qb : R.lq - R.qe;
    const long long cap = A.io.cigar_cap;
    uint32_t *const cg = A.io.cigar;
    auto put = [&](long long at, int op, int len) {
        if (lane == 0 && at >= 0 && at < cap) cg[at] = (uint32_t)len << 4 | (uint32_t)op;
    };
    if (clip5 > 0) put(base, 4, clip5);
    if (clip3 > 0) put(base + n_cigar - 1, 4, clip3);
    const long long first = base + (clip5 > 0);
    if (st.nodp) { put(first, 0, R.lQ); return; }
    long long have = 0;
    const unsigned char *const room = cg_room_of(A, k, &have);
    if (have <= 0) return;
    CgSeq S;
    S.q = A.io.qer + R.qoff + R.qb; S.t = A.io.text + R.rb; S.lQ = R.lQ; S.lT = R.lT; S.rev = R.is_rev;
    const int wb = cg_band(A.p, R.lQ, R.lT, A.io.alns[k].w);
    int mm = 0;
    const int n_core = st.n_core, squeeze = st.squeeze;
    cg_walk(S, wb, cg_room(R.lQ, R.lT, wb), room, lane, k, &mm, [&](int op, int len, int r) {
        int si = n_core - 1 - r;
        if (squeeze == 1) { if (si == 0) return; --si; }
        if (squeeze == 2 && r == 0) return;
        if (si >= 0 && si < n_cigar) put(first + si, op, len);
    });
}

struct CgLayout { size_t o_off, o_bsum, o_st, o_z; int blocks; };
CgLayout cg_layout(int64_t n)
{
    CgLayout L;
    const size_t nr = (size_t)n;
    L.blocks = mem_scan_blocks(n);
    L.o_off = 0;
    L.o_bsum = L.o_off + align256(2 * (nr + 1) * 8);
    L.o_st = L.o_bsum + align256(2 * (size_t)L.blocks * 8);
    L.o_z = L.o_st + align256(nr * sizeof(CgSt));
    return L;
}

}  // namespace

size_t mem_cigar_fixed_bytes(int64_t n) { return cg_layout(n < 0 ? 0 : n).o_z; }

size_t mem_cigar_record_z_bytes(const gbx_mem_cigar_params *p, int32_t lq, int32_t lt)
{
    if (lq < 1 || lt < 1 || p->w < 0 || p->w > (1 << 27) || p->e_del < 1 || p->e_ins < 1) return 0;
    const int w4 = 4 * p->w;
    return (size_t)cg_room_bytes(cg_room(lq, lt, cg_band(*p, lq, lt, w4)));
}

int mem_cigar_record_host(const gbx_mem_cigar_params *p, const gbx_bsw_seed &s, const gbx_bsw_seed_result &r, int64_t text_bytes,
                          int64_t qer_bytes, int64_t l_pac, size_t *z_need)
{
    const CgRec R = cg_record(s, r, text_bytes, qer_bytes, l_pac);
    *z_need = R.valid == 1 ? (size_t)cg_need(*p, R) : 0;
    return R.valid;
}

int mem_cigar_launch(const gbx_mem_cigar_params *p, int64_t n, const MemCigarIo &io, void *d_work, size_t work_bytes, int64_t z_bytes,
                     hipStream_t s)
{
    if (n >= (1ll << 31) - 1) { set_error("mem cigar: more than 2^31 - 2 records in one call"); return GBX_ERR_UNSUPPORTED; }
    const CgLayout L = cg_layout(n);
    if (z_bytes < 0 || work_bytes < L.o_z + (size_t)z_bytes) { set_error("mem cigar: workspace too small"); return GBX_ERR_ARG; }
    char *wb = (char *)d_work;
    CgArgs A;
    A.p = *p; A.io = io; A.n = n; A.z_bytes = z_bytes;
    A.off = (long long *)(wb + L.o_off); A.st = (CgSt *)(wb + L.o_st);
    A.z = (unsigned char *)(wb + L.o_z);
    auto scan = [&](int q) {                                     // off[q][0 .. n]; only the words' total leaves
        mem_scan_launch({A.off + q * (n + 1), n, 1, (long long *)(wb + L.o_bsum) + q * L.blocks, L.blocks, {q == 1 ? io.n_cigar : nullptr, nullptr},
                         nullptr, {}}, s);
    };
    {
        Stage st("mem_cigar_need", s);
        if (n > 0) hipLaunchKernelGGL(mem_cigar_need_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, A);
        scan(0);
    }
    if (n > 0) {
        Stage st("mem_cigar_align", s);
        hipLaunchKernelGGL(mem_cigar_align_kernel, dim3((unsigned)n), dim3(64), 0, s, A);
    }
    {
        Stage st("mem_cigar_scan", s);
        scan(1);
    }
    if (n > 0) {
        Stage st("mem_cigar_pack", s);
        hipLaunchKernelGGL(mem_cigar_pack_kernel, dim3((unsigned)n), dim3(64), 0, s, A);
    }
    GBX_HIP(hipGetLastError());
    GBX_GUARD_CHECK("mem cigar");
    return GBX_OK;
}

}  // namespace gbx
