// abea_eventalign_kernels.hip — f5c eventalign's realign_read for gfx950: align_read_to_ref (R/benchmarks/abea/src/
// eventalign.c:1263-1540) with profile_hmm_align, its Viterbi fill and its traceback (:345-911).
//
// One read per wavefront, drawn from a cursor over the caller's order (longest first).  The wavefront runs the read's whole
// chain of segments itself: plan a segment from the CIGAR, fill, trace back, emit up to 50 records, plan the next one where
// the last record ended.  Nothing goes to the host in between.
//
// Plan.  The aligned pairs are never materialised.  A prelude scans the CIGAR 64 operations at a time and keeps, for every
// aligned operation that survives the two trims, (ref_start, read_start, len, pairs before it).  ref_pos rises strictly along
// the pairs, so get_end_pair is "the last operation whose ref_start is at most x" and an offset into it; the starts only move
// forward from segment to segment, so the search is a 64-wide scan from a cursor.  get_closest_event_to reads the map and the
// nearest-k-mer table the record's count pass left (abea_dev.h).
//
// Fill.  The skew of abea_meth_kernel<64, 2>: lane l owns blocks 2l and 2l + 1 and works on row t - l at step t; what it needs
// of lane l - 1 arrives by three __shfl_up, the row before that is what arrived a step earlier.  Gaussians and the previous
// row live in registers, float max replaces p7_FLogsum, the scores are not kept.  A cell yields three movement codes (0..5);
// the nine bits of a block go into 16, a lane's two blocks into one 32-bit word, a row is 48 words = 192 bytes of the
// wavefront's slab in the workspace.  A segment has at most 96 k-mers, so 48 lanes carry it; there is no one-block-per-lane
// variant.
//
// Traceback.  The walk leaves a row on every step that is not K, so the rows it will visit are known: R, R - 1, ..., 1.  The
// wavefront loads them eight rows at a time, every lane its own word (coalesced 192-byte rows), with the next eight already
// in flight while the current eight are walked; a step of the walk is one __shfl of the row's registers and bit arithmetic,
// all lanes in lockstep.  K steps stay in the row and cost no load.  Lane i of a tile keeps the state of its row and the tile's
// records are written together.  Row rho emits event e_start + (rho - 1) * stride, so the records of rows 2 .. n_emit + 1 go
// straight to their slots and nothing is reversed.
//
// Every data-dependent loop is counted: segments <= n_events + 1, traceback steps <= rows + k-mers + 1, searches by the
// operation count.  A loop that hits its bound sets GBX_ABEA_EVENTALIGN_ST_BOUND and leaves the read.
#include <cmath>
#include "abea_dev.h"

namespace gbx {
namespace {

using abea_dev::rec_scan_incl;
using abea_dev::rec_closest;

constexpr int EA_MAXK = GBX_ABEA_EVENTALIGN_MAX_KMERS;
constexpr int EA_ROW_WORDS = EA_MAXK / 2;      // 32-bit words of a backtrack row
constexpr int EA_ALIGN_STRIDE = 100;           // align_stride, eventalign.c:1341
constexpr int EA_OUTPUT_STRIDE = 50;           // output_stride, eventalign.c:1342
constexpr int EA_TILE = 8;                     // rows of a traceback tile
constexpr int EA_SOFT = 5;                     // HMT_FROM_SOFT

// toupper, then disambiguate (eventalign.c:1054-1109): the lexicographically lowest base of an IUPAC code; any other byte: A
__device__ inline unsigned ea_rank(char c)
{
    if (c >= 'a' && c <= 'z') c -= 32;
    switch (c) {
    case 'C': case 'S': case 'Y': case 'B': return 1u;
    case 'G': case 'K': return 2u;
    case 'T': return 3u;
    default: return 0u;
    }
}

// update_cell, eventalign.c:621-633: the maximum of the six candidates in index order, `from` the last index that equals it
__device__ __forceinline__ float ea_pick(float x0, float x1, float x2, float x3, float x4, float x5, int &from)
{
    float mx = x0;
    int f = 0;
    mx = x1 > mx ? x1 : mx; f = mx == x1 ? 1 : f;
    mx = x2 > mx ? x2 : mx; f = mx == x2 ? 2 : f;
    mx = x3 > mx ? x3 : mx; f = mx == x3 ? 3 : f;
    mx = x4 > mx ? x4 : mx; f = mx == x4 ? 4 : f;
    mx = x5 > mx ? x5 : mx; f = mx == x5 ? 5 : f;
    from = f;
    return mx;
}

// The last operation at or behind `from` whose key (field 0: ref_start, else: the pairs before it) is at most x, with its
// entry in `out`; -1 when operation `from` itself lies above x.  The keys rise along the operations.
__device__ inline int ea_find(const int4 *ops, int n_ops, int from, int field, long long x, int lane, int4 &out)
{
    int res = -1;
    for (int o = max(from, 0); o < n_ops; o += 64) {
        const int idx = o + lane;
        const int4 v = idx < n_ops ? ops[idx] : make_int4(0, 0, 0, 0);
        const long long key = field ? v.w : v.x;
        const unsigned long long m = __ballot(idx < n_ops && key <= x);
        if (!m) break;
        const int hi = 63 - __clzll((long long)m);
        res = o + hi;
        out.x = __shfl(v.x, hi); out.y = __shfl(v.y, hi); out.z = __shfl(v.z, hi); out.w = __shfl(v.w, hi);
        if (hi < 63) break;
    }
    return res;
}

__device__ inline void ea_load_tile(uint32_t (&t)[EA_TILE], const uint32_t *bt, int top, int lane)
{
#pragma unroll
    for (int i = 0; i < EA_TILE; ++i) {
        const int row = top - i;
        t[i] = (row >= 1 && lane < EA_ROW_WORDS) ? bt[(size_t)(row - 1) * EA_ROW_WORDS + lane] : 0u;
    }
}

__device__ void ea_read(const AbeaEventalignArgs &A, long long r, int lane, uint32_t *bt, int4 *ops_all)
{
    int n_rec = 0, status = 0;
    long long n_seg = 0, n_cells = 0, n_steps = 0;
    const int read_len = A.seq_len[r], n_kmers = read_len - GBX_ABEA_KMER + 1;
    const long long e0 = A.event_off[r];
    const int ne = (int)min(A.event_off[r + 1] - e0, 0x3fffffffLL);
    const long long c0 = A.cigar_off[r];
    const long long n_cigar = min(A.cigar_off[r + 1], A.n_cigar_total) - c0;
    if ((A.flags && A.flags[r] != 0) || n_kmers < 1 || ne < 1 || c0 < 0 || n_cigar < 1) {
        if (lane == 0) {
            A.n_rec[r] = 0; A.status[r] = 0;
            if (A.counts) { A.counts[3 * r] = 0; A.counts[3 * r + 1] = 0; A.counts[3 * r + 2] = 0; }
        }
        return;
    }
    const int2 *mp = reinterpret_cast<const int2 *>(A.map) + A.seq_off[r];
    const int2 *nr = reinterpret_cast<const int2 *>(A.near) + A.seq_off[r];
    const long long pos = A.pos[r];
    const bool rev = A.rc[r] != 0;
    const char *ref = A.ref + A.ref_off[r];
    const int ref_len = A.ref_len[r];
    const float *ev = A.event_mean + e0;
    gbx_abea_eventalign_rec *rec = A.rec + e0;

    // ---- the aligned operations (get_aligned_segments_two_params, the two trims; eventalign.c:1112-1179, 932-957)
    const uint32_t *cig = A.cigar + c0;
    int4 *ops = ops_all + c0;
    const bool region = A.region_start != -1 && A.region_end != -1;
    const long long max_k = (long long)read_len - GBX_ABEA_KMER;
    int n_ops = 0;
    long long n_pairs = 0;
    {
        long long read_pos = 0, ref_adv = 0;
        for (long long c = 0; c < n_cigar; c += 64) {
            const bool live = c + lane < n_cigar;
            const uint32_t w = live ? cig[c + lane] : 0u;
            const long long len = live ? (long long)(w >> 4) : 0;
            const int op = (int)(w & 0xf);
            const bool aligned = op == 0 || op == 7 || op == 8;                   // M, =, X
            const long long rinc = (aligned || op == 1 || op == 4) ? len : 0;     // I and S advance the read
            const long long finc = (aligned || op == 2) ? len : 0;                // D advances the reference; H, and what is refused, nothing
            const long long ri = rec_scan_incl(rinc, lane), fi = rec_scan_incl(finc, lane);
            const long long rp = read_pos + ri - rinc, fp = pos + ref_adv + fi - finc;
            long long jlo = 0, jhi = len;
            if (region) { jlo = max(jlo, (long long)A.region_start - fp); jhi = min(jhi, (long long)A.region_end - fp + 1); }
            jhi = min(jhi, max_k - rp + 1);
            const int cnt = aligned && jhi > jlo ? (int)min(jhi - jlo, 0x3fffffffLL) : 0;
            const unsigned long long keep = __ballot(cnt > 0);
            const int idx = n_ops + __popcll(keep & ((1ull << lane) - 1ull));
            const long long ki = rec_scan_incl(cnt, lane);
            if (cnt > 0) ops[idx] = make_int4((int)(fp + jlo), (int)(rp + jlo), cnt, (int)min(n_pairs + ki - cnt, 0x7fffffffLL));
            n_ops += __popcll(keep);
            n_pairs += __shfl(ki, 63);
            read_pos += __shfl(ri, 63);
            ref_adv += __shfl(fi, 63);
        }
    }
    // the operations are read back by every lane: one wavefront, its own stores
    __threadfence_block();
    __syncthreads();

    const float sc = A.scale[r], sh = A.shift[r], vr = A.var[r], lv = A.log_var[r];
    const float *T = A.trans + (size_t)r * GBX_ABEA_METH_NTRANS;
    const float lp_mk = T[0], lp_mb = T[1], lp_mm_self = T[2], lp_mm_next = T[3], lp_bb = T[4], lp_bk = T[5], lp_bm_next = T[6],
                lp_bm_self = T[7], lp_kk = T[8], lp_km = T[9];
    const float NINF = -INFINITY;

    if (n_pairs > 0 && n_pairs < 0x7fffffffLL) {
        const int4 o_first = ops[0], o_last = ops[n_ops - 1];
        int k_start = o_first.y, k_end = o_last.y + o_last.z - 1;
        if (rev) { k_start = read_len - k_start - GBX_ABEA_KMER; k_end = read_len - k_end - GBX_ABEA_KMER; }
        const bool k_ok = k_start >= 0 && k_start < n_kmers && k_end >= 0 && k_end < n_kmers;
        const int first_event = k_ok ? rec_closest(mp, nr, k_start, n_kmers) : -1;
        const int last_event = k_ok ? rec_closest(mp, nr, k_end, n_kmers) : -1;
        if (first_event < 0 || last_event < 0 || first_event >= ne || last_event >= ne) {
            status |= GBX_ABEA_EVENTALIGN_ST_UNDEFINED;
        } else {
            const bool forward = first_event < last_event;
            int cse = first_event;                                              // curr_start_event
            long long csr = o_first.x;                                          // curr_start_ref
            long long cpi = 0;                                                  // curr_pair_idx
            int cop = 0;                                                        // the operation of pair cpi
            for (int seg = 0;; ++seg) {
                if (!(forward ? cse < last_event : cse > last_event)) break;
                if (seg > ne) { status |= GBX_ABEA_EVENTALIGN_ST_BOUND; break; }
                // get_end_pair(pairs, curr_start_ref + align_stride, curr_pair_idx), eventalign.c:919-928
                int4 v = make_int4(0, 0, 0, 0);
                int o = ea_find(ops, n_ops, cop, 0, csr + EA_ALIGN_STRIDE, lane, v);
                long long epi = o < 0 ? -1 : (long long)v.w + min((long long)v.z - 1, csr + EA_ALIGN_STRIDE - v.x);
                if (epi < cpi - 1) {                                            // the search starts at pair_idx and returns pair_idx - 1 at once
                    epi = cpi - 1;
                    o = epi < 0 ? -1 : ea_find(ops, n_ops, 0, 1, epi, lane, v);
                    if (o < 0) { status |= GBX_ABEA_EVENTALIGN_ST_UNDEFINED; break; }
                }
                const long long j = epi - v.w;
                const long long end_ref = (long long)v.x + j;
                int end_read = (int)(v.y + j);
                const bool last_section = epi == n_pairs - 1;
                if (rev) end_read = read_len - end_read - GBX_ABEA_KMER;
                const long long s = csr - pos, l = end_ref - csr + 1;
                if (l < 2 * GBX_ABEA_KMER) break;                               // also l <= 0: inside a deletion of more than 100 bases
                if (s < 0 || s + l > ref_len || l > EA_MAXK + GBX_ABEA_KMER - 1 || end_read < 0 || end_read >= n_kmers) {
                    status |= GBX_ABEA_EVENTALIGN_ST_UNDEFINED;
                    break;
                }
                const int stop = rec_closest(mp, nr, end_read, n_kmers);        // input_event_stop_idx
                if (abs(cse - stop) < 2) break;
                const int stride = cse < stop ? 1 : -1;
                if (stop < 0 || stop >= ne || (rev ? stride != -1 : stride != 1)) { status |= GBX_ABEA_EVENTALIGN_ST_UNDEFINED; break; }
                const int R = abs(stop - cse) + 1;                              // rows 1 .. R; row 0 is -inf
                const int nk = (int)l - GBX_ABEA_KMER + 1, nl = (nk + 1) >> 1;
                if (R > A.rows_cap) { status |= GBX_ABEA_EVENTALIGN_ST_ROWS; break; }
                const int n_emit = last_section ? R - 1 : min(R - 1, EA_OUTPUT_STRIDE);
                if (n_rec + n_emit > ne) { status |= GBX_ABEA_EVENTALIGN_ST_BOUND; break; }
                ++n_seg;
                n_cells += 3ll * R * nk;

                // ---- fill (profile_hmm_fill_generic_r9 with ProfileHMMViterbiOutputR9, eventalign.c:345-683)
                float gm[2], gs[2], gl[2], M[2], B[2], K[2];
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const int ki = min(lane * 2 + c, nk - 1);                   // blocks past the last k-mer are never updated
                    const char *p = ref + s + ki;
                    uint32_t rank = 0;
#pragma unroll
                    for (int i = 0; i < GBX_ABEA_KMER; ++i)                     // rc: the k-mer of the reverse-complement string, eventalign.c:436-444
                        rank = rank << 2 | (rev ? 3u - ea_rank(p[GBX_ABEA_KMER - 1 - i]) : ea_rank(p[i]));
                    const gbx_abea_model m = A.models[rank];
                    gm[c] = sc * m.level_mean + sh;                             // eventalign.c:320-330
                    gs[c] = m.level_stdv * vr;
                    gl[c] = -0.918938f - (m.level_log_stdv + lv);
                    M[c] = B[c] = K[c] = NINF;
                }
                const int steps = R + nl - 1;
                float pM = NINF, pB = NINF, pK = NINF;                          // lane l - 1's last block, the row before
                int rn = min(max(-lane, 0), R - 1);
                float x = ev[cse + rn * stride];
                for (int t = 0; t < steps; ++t) {
                    rn = min(max(t + 1 - lane, 0), R - 1);
                    const float xn = ev[cse + rn * stride];
                    float cM = __shfl_up(M[1], 1), cB = __shfl_up(B[1], 1), cK = __shfl_up(K[1], 1);
                    if (lane == 0) cM = cB = cK = NINF;                         // the start block
                    const int row = t - lane;                                   // 0-based; the reference's row - 1
                    if (lane < nl && row >= 0 && row < R) {
                        float dM = pM, dB = pB, dK = pK;                        // the block to the left, the row before
                        float sM = cM, sB = cB, sK = cK;                        // the block to the left, this row
                        uint32_t word = 0;
#pragma unroll
                        for (int c = 0; c < 2; ++c) {
                            const int ki = lane * 2 + c;
                            if (ki < nk) {
                                const float a = (x - gm[c]) / gs[c];                                    // eventalign.c:297-298
                                const float em = gl[c] + (-0.5f * a * a);
                                int fM, fB, fK;
                                const float soft = (ki == 0 && row == 0) ? 0.0f + A.pre0 : NINF;        // eventalign.c:521-523, hmm_flags = 0
                                const float mn = ea_pick(lp_mm_self + M[c], lp_mm_next + dM, lp_bm_self + B[c], lp_bm_next + dB, lp_km + dK, soft, fM) + em;
                                const float bn = ea_pick(lp_mb + M[c], NINF, lp_bb + B[c], NINF, NINF, NINF, fB) + 0.0f;
                                const float kn = ea_pick(NINF, lp_mk + sM, NINF, lp_bk + sB, lp_kk + sK, NINF, fK) + 0.0f;
                                dM = M[c]; dB = B[c]; dK = K[c];
                                M[c] = sM = mn; B[c] = sB = bn; K[c] = sK = kn;
                                word |= (uint32_t)(fM | fB << 3 | fK << 6) << (16 * c);
                            }
                        }
                        pM = cM; pB = cB; pK = cK;
                        bt[(size_t)row * EA_ROW_WORDS + lane] = word;
                    }
                    x = xn;
                }
                // the traceback starts at M of the last k-mer in the last row and asserts that it is not -inf (eventalign.c:809-828)
                const float fin = __shfl(((nk - 1) & 1) ? M[1] : M[0], (nk - 1) >> 1);
                if (!(fin > NINF)) { status |= GBX_ABEA_EVENTALIGN_ST_UNDEFINED; break; }
                __threadfence_block();
                __syncthreads();

                // ---- traceback and emission (eventalign.c:815-886, 1463-1514)
                int row = R, kmer = nk - 1, st = 0;                             // st: 0 M, 1 B, 2 K
                int last_k = -1, tsteps = 0;
                bool done = false, bad = false;
                const int max_steps = R + nk + 1;
                uint32_t cur[EA_TILE], nxt[EA_TILE];
                ea_load_tile(cur, bt, R, lane);
                for (int top = R; top >= 1 && !done && !bad; top -= EA_TILE) {
                    ea_load_tile(nxt, bt, top - EA_TILE, lane);
                    int myk = 0, myst = 0, myrow = 0;
#pragma unroll
                    for (int i = 0; i < EA_TILE; ++i) {
                        if (done || bad || row != top - i || row < 1) continue;
                        for (;;) {                                              // the K steps of a row, then the step that leaves it
                            if (++tsteps > max_steps) { bad = true; status |= GBX_ABEA_EVENTALIGN_ST_BOUND; break; }
                            const uint32_t w = __shfl(cur[i], kmer >> 1);
                            const int code = (int)(w >> ((kmer & 1) * 16 + 3 * st)) & 7;
                            if (st != 2) {
                                if (lane == i) { myk = kmer; myst = st; myrow = row; }
                                if (row == n_emit + 1) last_k = kmer;
                            }
                            if (code == EA_SOFT) { done = true; break; }
                            const int was = st;
                            st = code <= 1 ? 0 : code == 4 ? 2 : 1;
                            if (code == 1 || code == 3 || code == 4) --kmer;
                            if (kmer < 0 || code > EA_SOFT) { bad = true; break; }
                            if (was != 2) { --row; break; }
                        }
                    }
                    if (lane < EA_TILE && myrow >= 2 && myrow - 2 < n_emit) {
                        gbx_abea_eventalign_rec q;
                        q.ref_pos = (int32_t)(csr + myk);
                        q.event_idx = cse + (myrow - 1) * stride;
                        q.state = myst == 0 ? 'M' : 'B';
                        rec[n_rec + myrow - 2] = q;
                    }
#pragma unroll
                    for (int i = 0; i < EA_TILE; ++i) cur[i] = nxt[i];
                }
                n_steps += tsteps;
                // a finite path ends by HMT_FROM_SOFT in row 1 (the only finite way in); anything else left the matrix
                if (bad || !done || row != 1 || last_k < 0) { status |= (status & GBX_ABEA_EVENTALIGN_ST_BOUND) ? 0 : GBX_ABEA_EVENTALIGN_ST_UNDEFINED; break; }
                n_rec += n_emit;
                cse += n_emit * stride;                                         // last_event_output
                csr += last_k;                                                  // last_ref_kmer_output
                // curr_pair_idx = get_end_pair(pairs, curr_start_ref, curr_pair_idx)
                o = ea_find(ops, n_ops, cop, 0, csr, lane, v);
                long long npi = o < 0 ? -1 : (long long)v.w + min((long long)v.z - 1, csr - v.x);
                if (npi < cpi - 1) {
                    npi = cpi - 1;
                    o = npi < 0 ? -1 : ea_find(ops, n_ops, 0, 1, npi, lane, v);
                }
                cpi = max(npi, 0ll);
                cop = max(o, 0);
                if (n_emit == 0) break;
                // the slab is rewritten by the next fill: this segment's loads are done, its stores ordered behind them
                __syncthreads();
            }
        }
    }
    if (lane == 0) {
        A.n_rec[r] = n_rec; A.status[r] = status;
        if (A.counts) { A.counts[3 * r] = n_seg; A.counts[3 * r + 1] = n_cells; A.counts[3 * r + 2] = n_steps; }
    }
}

__global__ void __launch_bounds__(64) abea_eventalign_kernel(AbeaEventalignArgs A, size_t ops_bytes)
{
    const int lane = threadIdx.x;
    unsigned long long *cursor = reinterpret_cast<unsigned long long *>(A.work);
    int4 *ops_all = reinterpret_cast<int4 *>(reinterpret_cast<char *>(A.work) + 256);
    uint32_t *bt = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(A.work) + 256 + ops_bytes) + (size_t)blockIdx.x * A.rows_cap * EA_ROW_WORDS;
    for (long long it = 0; it < A.n_reads; ++it) {
        unsigned long long slot = 0;
        if (lane == 0) slot = atomicAdd(cursor, 1ull);
        slot = __shfl(slot, 0);
        if (slot >= (unsigned long long)A.n_reads) break;
        const long long r = A.order ? A.order[slot] : (long long)slot;
        if (r < 0 || r >= A.n_reads) continue;
        ea_read(A, r, lane, bt, ops_all);
        __syncthreads();
    }
}

inline size_t ea_ops_bytes(int64_t n_cigar_total) { return ((size_t)std::max<int64_t>(n_cigar_total, 0) * sizeof(int4) + 255) & ~(size_t)255; }

}  // namespace

size_t abea_eventalign_workspace_bytes(int64_t n_reads, int64_t n_cigar_total, int64_t rows_cap)
{
    const size_t slabs = (size_t)std::min<int64_t>(std::max<int64_t>(n_reads, 1), GBX_ABEA_EVENTALIGN_SLABS);
    return 256 + ea_ops_bytes(n_cigar_total) + slabs * (size_t)std::max<int64_t>(rows_cap, 1) * EA_ROW_WORDS * 4;
}

int abea_eventalign_launch(AbeaEventalignArgs a, size_t work_bytes, hipStream_t s)
{
    if (a.n_reads == 0) return GBX_OK;
    if (a.n_reads > 0x7fffffffLL - 1024) { set_error("abea eventalign: more than 2^31 reads in one call"); return GBX_ERR_UNSUPPORTED; }
    if (a.rows_cap < 1 || a.rows_cap > 0x00ffffffLL) { set_error("abea eventalign: rows_cap %lld", a.rows_cap); return GBX_ERR_ARG; }
    const size_t ops_bytes = ea_ops_bytes(a.n_cigar_total), slab = (size_t)a.rows_cap * EA_ROW_WORDS * 4;
    if (work_bytes < 256 + ops_bytes + slab) {
        set_error("abea eventalign: workspace of %zu bytes, %zu needed for one wavefront", work_bytes, 256 + ops_bytes + slab);
        return GBX_ERR_ARG;
    }
    const long long fit = (long long)((work_bytes - 256 - ops_bytes) / slab);
    const long long grid = std::min<long long>(std::min<long long>(a.n_reads, GBX_ABEA_EVENTALIGN_SLABS), fit);
    a.pre0 = (float)log(1 - 0.5);                                              // TRANS_START_TO_CLIP, eventalign.c:25, 124
    GBX_HIP(hipMemsetAsync(a.work, 0, 256, s));
    Stage st("abea_eventalign", s);
    hipLaunchKernelGGL(abea_eventalign_kernel, dim3((unsigned)grid), dim3(64), 0, s, a, ops_bytes);
    GBX_HIP(hipGetLastError());
    return GBX_OK;
}

}  // namespace gbx
