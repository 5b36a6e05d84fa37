// capi_bsw_seeds.hip — whole-seed extension (include/gbx.h: gbx_bsw_extend_seeds_*): bwa-mem2's extension caller
// (mem_chain2aln's two ksw_extend2 calls with MAX_BAND_TRY) on the device, as a chain of small kernels around the existing
// bsw launch.  Per call, all on one stream and without a host round trip:
//   prep       both arenas reversed into the workspace, the left (reversed) and right (forward) pair descriptors
//   per side, per band try i:  bsw_launch over all n pairs with band w << i, then bsw_seed_retry_kernel: a seed that is
//              done (or was never extended on this side) gets an empty pair, which the next launch's classify answers
//              without DP
//   hand-off   the left local-vs-to-end choice, sc0 into the right descriptors' h0
//   finalize   the right choice, gbx_bsw_seed_result
// The host entry uploads, runs the device entry on its lane's stream and downloads.  It does not use the call combiner, the
// multi-device layer or the chunked transfer pipeline of the pair entries (host_combine.h, host_multi.h, host_pipeline.h):
// possible later, one device and one stream per call for now.
#include "capi_common.h"

using namespace gbx;

namespace {

static_assert(sizeof(gbx_bsw_seed) == 40 && sizeof(gbx_bsw_seed_result) == 32, "gbx.h seed structs");

// One side's pair descriptors (bsw_launch's flat arrays) and its latest result per seed.
struct SideArrays {
    int64_t *idr, *idq;
    int32_t *len1, *len2, *h0, *aw;     // aw: the band of the side's last try (w until a try runs)
    gbx_bsw_result *res;
};

// Workspace: reversed ref | reversed qer | left side | right side | launch output | bsw_launch's own workspace.  A reversed
// arena is the source rounded up to 16 bytes and reversed whole (its first `lead` = padded - bytes bytes come from past the
// end), followed by 16 zero bytes of slack.
struct SeedWork {
    uint8_t *rref, *rqer;
    int64_t lead_r, lead_q, vec_r, vec_q;       // vec_*: 16-byte vectors of the padded source
    SideArrays side[2];
    gbx_bsw_result *launch_out;
    void *bsw_work;
    size_t bsw_work_bytes, total;
};

constexpr size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

SeedWork seed_work_layout(char *base, int64_t n, int64_t ref_bytes, int64_t qer_bytes)
{
    SeedWork W;
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = base ? base + off : nullptr; off += al256(bytes); return p; };
    const int64_t pr = (ref_bytes + 15) & ~(int64_t)15, pq = (qer_bytes + 15) & ~(int64_t)15;
    W.lead_r = pr - ref_bytes; W.lead_q = pq - qer_bytes;
    W.vec_r = pr / 16; W.vec_q = pq / 16;
    W.rref = (uint8_t *)take((size_t)pr + 16);
    W.rqer = (uint8_t *)take((size_t)pq + 16);
    const size_t m = (size_t)(n > 0 ? n : 0);
    for (SideArrays &s : W.side) {
        s.idr = (int64_t *)take(m * 8); s.idq = (int64_t *)take(m * 8);
        s.len1 = (int32_t *)take(m * 4); s.len2 = (int32_t *)take(m * 4); s.h0 = (int32_t *)take(m * 4); s.aw = (int32_t *)take(m * 4);
        s.res = (gbx_bsw_result *)take(m * sizeof(gbx_bsw_result));
    }
    W.launch_out = (gbx_bsw_result *)take(m * sizeof(gbx_bsw_result));
    W.bsw_work_bytes = bsw_workspace_bytes(n);
    W.bsw_work = take(W.bsw_work_bytes);
    W.total = off;
    return W;
}

// What the host entry checks per seed (0 = fine, 1 = argument error, 2 = beyond the length limits); the prep kernel applies the
// same rule to the seeds the device entry is given.
__host__ __device__ inline int seed_check(const gbx_bsw_seed &s, int64_t ref_bytes, int64_t qer_bytes)
{
    const int64_t qend = (int64_t)s.qbeg + s.len, rend = (int64_t)s.rbeg + s.len;
    if (s.qbeg < 0 || s.len < 1 || qend > s.lq || s.rbeg < 0 || rend > s.rlen || s.qoff < 0 || s.roff < 0 ||
        s.qoff > qer_bytes - s.lq || s.roff > ref_bytes - s.rlen)
        return 1;
    if (s.qbeg > GBX_BSW_MAX_QLEN || s.rbeg > GBX_BSW_MAX_TLEN || s.lq - qend > GBX_BSW_MAX_QLEN || s.rlen - rend > GBX_BSW_MAX_TLEN)
        return 2;
    return 0;
}

// 16 bytes reversed: the four dwords in reverse order, each byte-swapped (v_perm_b32)
__device__ inline uint4 rev16(uint4 v)
{
    return make_uint4(__builtin_bswap32(v.w), __builtin_bswap32(v.z), __builtin_bswap32(v.y), __builtin_bswap32(v.x));
}

__device__ inline void reverse_vec(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, int64_t nvec, int64_t v, bool aligned)
{
    if (v > nvec) return;
    if (v == nvec) { *(uint4 *)(dst + 16 * v) = make_uint4(0, 0, 0, 0); return; }      // slack
    const int64_t from = nvec - 1 - v;
    if (aligned) {
        *(uint4 *)(dst + 16 * v) = rev16(*(const uint4 *)(src + 16 * from));
    } else {
        for (int b = 0; b < 16; ++b) dst[16 * v + b] = src[16 * from + 15 - b];
    }
}

constexpr int SEED_THREADS = 256;

// One pass over max(vectors of either arena + 1, seeds): reversal and the descriptors.
__global__ void __launch_bounds__(SEED_THREADS) bsw_seed_prep_kernel(const uint8_t *ref, const uint8_t *qer, const gbx_bsw_seed *__restrict__ seeds,
                                                                      int64_t n, int64_t ref_bytes, int64_t qer_bytes, SeedWork W, int a, int w,
                                                                      int aligned, int64_t total, gbx_bsw_seed_result *__restrict__ out)
{
    const int64_t stride = (int64_t)gridDim.x * SEED_THREADS;
    for (int64_t t = (int64_t)blockIdx.x * SEED_THREADS + threadIdx.x; t < total; t += stride) {
        reverse_vec(ref, W.rref, W.vec_r, t, aligned & 1);
        reverse_vec(qer, W.rqer, W.vec_q, t, aligned & 2);
        if (t >= n) continue;
        const gbx_bsw_seed s = seeds[t];
        const int bad = seed_check(s, ref_bytes, qer_bytes);
        const int q0 = s.qbeg + s.len, r0 = s.rbeg + s.len;
        SideArrays L = W.side[0], R = W.side[1];
        // left: reverse(win[0:rbeg]) = rref[lead + ref_bytes - roff - rbeg, + rbeg), likewise the read's prefix
        L.idr[t] = W.lead_r + ref_bytes - s.roff - s.rbeg;
        L.idq[t] = W.lead_q + qer_bytes - s.qoff - s.qbeg;
        const bool left = !bad && s.qbeg > 0, right = !bad && q0 != s.lq;
        L.len1[t] = left ? s.rbeg : 0; L.len2[t] = left ? s.qbeg : 0; L.h0[t] = s.len * a;
        R.idr[t] = s.roff + r0; R.idq[t] = s.qoff + q0;
        R.len1[t] = right ? s.rlen - r0 : 0; R.len2[t] = right ? s.lq - q0 : 0; R.h0[t] = 0;
        L.aw[t] = w; R.aw[t] = w;
        if (bad) { gbx_bsw_seed_result r = {-1, -1, -1, -1, -1, -1, -1, -1}; out[t] = r; }
    }
}

// After a side's try i with band aw: a seed extended in this try keeps the result; it is done when the score did not change or
// max_off < aw/2 + aw/4 (or no try is left), and a done seed's pair becomes empty for the next try.  The first try's
// "previous score" is -1 on the left and sc0 (the right pair's h0) on the right.
__global__ void __launch_bounds__(SEED_THREADS) bsw_seed_retry_kernel(SideArrays S, const gbx_bsw_result *__restrict__ got, int64_t n,
                                                                       int first_prev_is_h0, int try_i, int aw, int last)
{
    const int64_t k = (int64_t)blockIdx.x * SEED_THREADS + threadIdx.x;
    if (k >= n || S.len2[k] == 0) return;
    const gbx_bsw_result r = got[k];
    const int prev = try_i ? S.res[k].score : first_prev_is_h0 ? S.h0[k] : -1;
    S.res[k] = r;
    S.aw[k] = aw;
    if (last || r.score == prev || r.max_off < (aw >> 1) + (aw >> 2)) { S.len1[k] = 0; S.len2[k] = 0; }
}

// The left choice; sc0 into the right pairs' h0.  Partial results go to `out` (finalize completes them).
__global__ void __launch_bounds__(SEED_THREADS) bsw_seed_handoff_kernel(const gbx_bsw_seed *__restrict__ seeds, int64_t n, int64_t ref_bytes,
                                                                         int64_t qer_bytes, SideArrays L, SideArrays R, int a, int pen_clip5,
                                                                         gbx_bsw_seed_result *__restrict__ out)
{
    const int64_t k = (int64_t)blockIdx.x * SEED_THREADS + threadIdx.x;
    if (k >= n) return;
    const gbx_bsw_seed s = seeds[k];
    if (seed_check(s, ref_bytes, qer_bytes)) return;
    gbx_bsw_seed_result o;
    if (s.qbeg > 0) {
        const gbx_bsw_result r = L.res[k];
        o.score = r.score;
        if (r.gscore <= 0 || r.gscore <= r.score - pen_clip5) { o.qb = s.qbeg - r.qle; o.rb = s.rbeg - r.tle; o.truesc = r.score; }
        else { o.qb = 0; o.rb = s.rbeg - r.gtle; o.truesc = r.gscore; }
    } else {
        o.score = o.truesc = s.len * a; o.qb = 0; o.rb = s.rbeg;
    }
    o.sc0 = o.score;
    o.qe = o.re = o.w = 0;
    R.h0[k] = o.sc0;
    out[k] = o;
}

__global__ void __launch_bounds__(SEED_THREADS) bsw_seed_finalize_kernel(const gbx_bsw_seed *__restrict__ seeds, int64_t n, int64_t ref_bytes,
                                                                          int64_t qer_bytes, SideArrays L, SideArrays R, int pen_clip3,
                                                                          gbx_bsw_seed_result *__restrict__ out)
{
    const int64_t k = (int64_t)blockIdx.x * SEED_THREADS + threadIdx.x;
    if (k >= n) return;
    const gbx_bsw_seed s = seeds[k];
    if (seed_check(s, ref_bytes, qer_bytes)) return;
    gbx_bsw_seed_result o = out[k];
    const int q0 = s.qbeg + s.len, r0 = s.rbeg + s.len;
    if (q0 != s.lq) {
        const gbx_bsw_result r = R.res[k];
        o.score = r.score;
        if (r.gscore <= 0 || r.gscore <= r.score - pen_clip3) { o.qe = q0 + r.qle; o.re = r0 + r.tle; o.truesc += r.score - o.sc0; }
        else { o.qe = s.lq; o.re = r0 + r.gtle; o.truesc += r.gscore - o.sc0; }
    } else {
        o.qe = s.lq; o.re = r0;
    }
    o.w = max(L.aw[k], R.aw[k]);
    out[k] = o;
}

int seed_params_check(const char *who, const gbx_bsw_seed_params *p)
{
    if (p->max_band_try < 1 || p->max_band_try > 4) {
        set_error("%s: max_band_try must be in 1..4 (got %d)", who, p->max_band_try);
        return GBX_ERR_ARG;
    }
    if (p->bsw.w < 0 || p->bsw.w > (0x7fffffff >> (p->max_band_try - 1))) {
        set_error("%s: band w=%d out of range for max_band_try=%d", who, p->bsw.w, p->max_band_try);
        return GBX_ERR_ARG;
    }
    BswLaneRule rule;
    if (bsw_lane_rule(&p->bsw, 0, &rule) != GBX_OK) {     // the pair launch's own parameter check, without a device
        const std::string e = gbx_last_error();
        set_error("%s: %s", who, e.c_str());
        return GBX_ERR_ARG;
    }
    return GBX_OK;
}

int seeds_device(const gbx_bsw_seed_params *p, int64_t n, const uint8_t *d_ref, int64_t ref_bytes, const uint8_t *d_qer,
                 int64_t qer_bytes, const gbx_bsw_seed *d_seeds, gbx_bsw_seed_result *d_out, void *d_work, size_t work_bytes,
                 hipStream_t s)
{
    static const char *who = "gbx_bsw_extend_seeds_device";
    if (!p || n < 0 || ref_bytes < 0 || qer_bytes < 0) { set_error("%s: bad argument", who); return GBX_ERR_ARG; }
    int rc = seed_params_check(who, p);
    if (rc) return rc;
    if (n == 0) return GBX_OK;
    if (!d_ref || !d_qer || !d_seeds || !d_out || !d_work) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    if ((uintptr_t)d_work & 15) { set_error("%s: workspace not 16-byte aligned", who); return GBX_ERR_ARG; }
    if (n > 0x7fffffffLL - 1024) { set_error("%s: more than 2^31 seeds in one call", who); return GBX_ERR_UNSUPPORTED; }
    SeedWork W = seed_work_layout((char *)d_work, n, ref_bytes, qer_bytes);
    if (work_bytes < W.total) { set_error("%s: workspace too small (%zu < %zu bytes)", who, work_bytes, W.total); return GBX_ERR_ARG; }
    if ((rc = require_device())) return rc;
    const int a = p->bsw.mat[0];
    const int aligned = (((uintptr_t)d_ref & 15) == 0 ? 1 : 0) | (((uintptr_t)d_qer & 15) == 0 ? 2 : 0);
    int64_t total = W.vec_r > W.vec_q ? W.vec_r : W.vec_q;
    total = total + 1 > n ? total + 1 : n;
    const int64_t want = (total + SEED_THREADS - 1) / SEED_THREADS;
    const int blocks = (int)(want < 8192 ? want : 8192);
    const int sblocks = (int)((n + SEED_THREADS - 1) / SEED_THREADS);
    {
        Stage st("bsw_seed_prep", s);
        hipLaunchKernelGGL(bsw_seed_prep_kernel, dim3(blocks), dim3(SEED_THREADS), 0, s, d_ref, d_qer, d_seeds, n, ref_bytes, qer_bytes, W,
                           a, p->bsw.w, aligned, total, d_out);
        GBX_HIP(hipGetLastError());
    }
    gbx_bsw_params q = p->bsw;
    for (int side = 0; side < 2; ++side) {
        const SideArrays &S = W.side[side];
        const uint8_t *rf = side ? d_ref : W.rref, *qr = side ? d_qer : W.rqer;
        q.end_bonus = side ? p->pen_clip3 : p->pen_clip5;
        for (int i = 0; i < p->max_band_try; ++i) {
            q.w = p->bsw.w << i;
            if ((rc = bsw_launch(&q, n, rf, qr, S.idr, S.idq, S.len1, S.len2, S.h0, W.launch_out, W.bsw_work, W.bsw_work_bytes, s)))
                return rc;
            Stage st("bsw_seed_retry", s);
            hipLaunchKernelGGL(bsw_seed_retry_kernel, dim3(sblocks), dim3(SEED_THREADS), 0, s, S, (const gbx_bsw_result *)W.launch_out, n,
                               side, i, q.w, i == p->max_band_try - 1 ? 1 : 0);
            GBX_HIP(hipGetLastError());
        }
        if (side == 0) {
            Stage st("bsw_seed_handoff", s);
            hipLaunchKernelGGL(bsw_seed_handoff_kernel, dim3(sblocks), dim3(SEED_THREADS), 0, s, d_seeds, n, ref_bytes, qer_bytes,
                               W.side[0], W.side[1], a, p->pen_clip5, d_out);
            GBX_HIP(hipGetLastError());
        }
    }
    Stage st("bsw_seed_finalize", s);
    hipLaunchKernelGGL(bsw_seed_finalize_kernel, dim3(sblocks), dim3(SEED_THREADS), 0, s, d_seeds, n, ref_bytes, qer_bytes, W.side[0],
                       W.side[1], p->pen_clip3, d_out);
    GBX_HIP(hipGetLastError());
    return GBX_OK;
}

}  // namespace

extern "C" {

void gbx_bsw_seed_default_params(gbx_bsw_seed_params *p)
{
    memset(p, 0, sizeof(*p));
    gbx_bsw_default_params(&p->bsw);
    p->pen_clip5 = p->pen_clip3 = 5;
    p->max_band_try = 2;
}

size_t gbx_bsw_seeds_workspace_bytes(int64_t n, int64_t ref_bytes, int64_t qer_bytes)
{
    if (n < 0 || ref_bytes < 0 || qer_bytes < 0) return 0;
    return seed_work_layout(nullptr, n, ref_bytes, qer_bytes).total;
}

int gbx_bsw_extend_seeds_device(const gbx_bsw_seed_params *p, int64_t n,
                                const uint8_t *d_ref, int64_t ref_bytes, const uint8_t *d_qer, int64_t qer_bytes,
                                const gbx_bsw_seed *d_seeds, gbx_bsw_seed_result *d_out,
                                void *d_work, size_t work_bytes, void *stream)
{
    RoctxRange range_("gbx_bsw_extend_seeds_device");
    return seeds_device(p, n, d_ref, ref_bytes, d_qer, qer_bytes, d_seeds, d_out, d_work, work_bytes, (hipStream_t)stream);
}

int gbx_bsw_extend_seeds_host(const gbx_bsw_seed_params *p, int64_t n,
                              const uint8_t *ref, int64_t ref_bytes, const uint8_t *qer, int64_t qer_bytes,
                              const gbx_bsw_seed *seeds, gbx_bsw_seed_result *out)
{
    RoctxRange range_("gbx_bsw_extend_seeds_host");
    static const char *who = "gbx_bsw_extend_seeds_host";
    if (!p || n < 0 || ref_bytes < 0 || qer_bytes < 0) { set_error("%s: bad argument", who); return GBX_ERR_ARG; }
    int rc = seed_params_check(who, p);
    if (rc) return rc;
    if (n == 0) return GBX_OK;
    if (!ref || !qer || !seeds || !out) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
    for (int64_t k = 0; k < n; ++k) {                     // everything is checked before a device is touched
        const int bad = seed_check(seeds[k], ref_bytes, qer_bytes);
        if (bad == 1) {
            const gbx_bsw_seed &s = seeds[k];
            set_error("%s: seed %lld breaks the seed rules (qoff=%lld roff=%lld lq=%d rlen=%d qbeg=%d rbeg=%d len=%d; arenas %lld / %lld bytes)",
                      who, (long long)k, (long long)s.qoff, (long long)s.roff, s.lq, s.rlen, s.qbeg, s.rbeg, s.len,
                      (long long)qer_bytes, (long long)ref_bytes);
            return GBX_ERR_ARG;
        }
        if (bad == 2) {
            set_error("%s: seed %lld: a side exceeds GBX_BSW_MAX_QLEN/TLEN", who, (long long)k);
            return GBX_ERR_UNSUPPORTED;
        }
    }
    if ((rc = require_device())) return rc;
    HostLane lane;
    if ((rc = lane.acquire())) return rc;
    Lane *L = lane.l;
    const size_t wb = gbx_bsw_seeds_workspace_bytes(n, ref_bytes, qer_bytes);
    DevBuf dref(L), dqer(L), dseeds(L), dout(L), dwork(L);
    if ((rc = dref.alloc((size_t)ref_bytes)) || (rc = dqer.alloc((size_t)qer_bytes)) || (rc = dseeds.alloc((size_t)n * sizeof(gbx_bsw_seed))) ||
        (rc = dout.alloc((size_t)n * sizeof(gbx_bsw_seed_result))) || (rc = dwork.alloc(wb)))
        return rc;
    const hipStream_t s = L->compute;
    GBX_HIP(hipMemcpyAsync(dref.p, ref, (size_t)ref_bytes, hipMemcpyHostToDevice, s));
    GBX_HIP(hipMemcpyAsync(dqer.p, qer, (size_t)qer_bytes, hipMemcpyHostToDevice, s));
    GBX_HIP(hipMemcpyAsync(dseeds.p, seeds, (size_t)n * sizeof(gbx_bsw_seed), hipMemcpyHostToDevice, s));
    if ((rc = seeds_device(p, n, dref.as<uint8_t>(), ref_bytes, dqer.as<uint8_t>(), qer_bytes, dseeds.as<gbx_bsw_seed>(),
                           dout.as<gbx_bsw_seed_result>(), dwork.p, wb, s))) {
        (void)hipStreamSynchronize(s);                    // nothing of this call may still run when its buffers go back to the lane
        return rc;
    }
    GBX_HIP(hipMemcpyAsync(out, dout.p, (size_t)n * sizeof(gbx_bsw_seed_result), hipMemcpyDeviceToHost, s));
    GBX_HIP(hipStreamSynchronize(s));
    return GBX_OK;
}

}  // extern "C"
