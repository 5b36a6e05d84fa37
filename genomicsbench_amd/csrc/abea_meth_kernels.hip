// abea_meth_kernels.hip — the profile HMM score of f5c call-methylation (R/benchmarks/abea/src/hmm.c:301-727) for gfx950.
//
// One job = one profile_hmm_score call: rows (events) x blocks (k-mers) x 3 states (M match, B bad event, K k-mer skip).
// M and B of a cell read the previous row only; K reads K of the block to its left in the SAME row (hmm.c:467-474), so a
// row is a serial chain and the only parallelism inside a job is the anti-diagonal.  A job is therefore skewed over a group
// of W lanes: lane l owns C consecutive blocks and works on row t - l at step t, so that what it needs of lane l - 1 (the
// three states of that lane's last block, for this row and the one before) was finished one and two steps earlier.  Three
// shuffles per step hand them over; the values of the row before are the ones received a step earlier.  Everything of a
// job lives in registers (C is a template parameter, all block loops are unrolled); only the event mean and the two flank
// entries of the next step are fetched from memory, one step ahead.
//
// Every log-sum is p7_FLogsum (logsum.h:61-71): its 16 000-entry table sits in LDS, 64 000 bytes per work-group of 512
// lanes, two work-groups per CU.  The candidates of a cell are folded in the reference's order (hmm.c:558-566); folds with
// a -inf constant return the other operand unchanged and are left out.
//
// Jobs are plentiful (hundreds per read), so the grid is a counted loop over the jobs of a class: class c = (W, C) by k-mer
// count, sorted longest first on the host, consecutive jobs in the same wavefront.
#include "gbx_internal.h"

namespace gbx {
namespace {

constexpr int METH_BLOCK = 512;
constexpr int METH_TBL = GBX_ABEA_FLOGSUM_TBL;
constexpr int METH_MAX_GRID = 512;            // two work-groups per CU (LDS) x 256 CUs

__device__ __forceinline__ float meth_logsum(float a, float b, const float *tbl)
{
    const float mx = a > b ? a : b;
    const float mn = a < b ? a : b;
    const float d = mx - mn;
    const bool plain = mn == -INFINITY || d >= 15.7f;
    int idx = plain ? 0 : (int)(d * 1000.f);
    idx = min(max(idx, 0), METH_TBL - 1);     // a NaN score (events_per_base <= 1) must not index outside the table
    return plain ? mx : mx + tbl[idx];
}

__device__ __forceinline__ uint32_t meth_rank(char b)      // hmm.c:21-36
{
    return b == 'C' ? 1u : b == 'G' ? 2u : b == 'M' ? 3u : b == 'T' ? 4u : 0u;
}

template <int W, int C>
__global__ __launch_bounds__(METH_BLOCK) void abea_meth_kernel(long long n, const int32_t *__restrict__ order,
                                                               const gbx_abea_meth_job *__restrict__ jobs, const char *__restrict__ seq,
                                                               const int64_t *__restrict__ event_off, const float *__restrict__ event_mean,
                                                               const float *__restrict__ scale, const float *__restrict__ shift,
                                                               const float *__restrict__ var, const float *__restrict__ log_var,
                                                               const gbx_abea_model *__restrict__ model, const float *__restrict__ flogsum,
                                                               const float *__restrict__ trans, const float *__restrict__ pre_flank,
                                                               const float *__restrict__ post_flank, float *__restrict__ scores)
{
    __shared__ float tbl[METH_TBL];
    for (int i = threadIdx.x; i < METH_TBL; i += METH_BLOCK) tbl[i] = flogsum[i];
    __syncthreads();
    constexpr int GPW = 64 / W;                              // jobs of a wavefront
    constexpr int WPB = METH_BLOCK / 64;                     // wavefronts of a work-group
    const int l = threadIdx.x % W;
    const long long tasks = (n + GPW - 1) / GPW, per_round = (long long)gridDim.x * WPB;
    const long long n_rounds = (tasks + per_round - 1) / per_round;
    const float NINF = -INFINITY;
    for (long long round = 0; round < n_rounds; ++round) {
        const long long task = (round * gridDim.x + blockIdx.x) * WPB + threadIdx.x / 64;
        if (task >= tasks) continue;                         // the whole wavefront
        const long long slot = task * GPW + (threadIdx.x % 64) / W;
        const bool have = slot < n;                          // a group without a job runs the last job's loads and keeps nothing
        const int32_t jid = order[have ? slot : n - 1];
        const gbx_abea_meth_job J = jobs[jid];
        const int L = J.seq_len, nk = L - GBX_ABEA_KMER + 1, nl = (nk + C - 1) / C;
        const int rows = J.event_stop > J.event_start ? J.event_stop - J.event_start + 1 : J.event_start - J.event_stop + 1;
        const int stride = J.rc ? -1 : 1;
        const int r = J.read;
        const float *ev = event_mean + event_off[r] + J.event_start;
        const float sc = scale[r], sh = shift[r], vr = var[r], lv = log_var[r];
        const float *T = trans + (size_t)r * GBX_ABEA_METH_NTRANS;
        const float lp_mk = T[0], lp_mb = T[1], lp_mm_self = T[2], lp_mm_next = T[3], lp_bb = T[4], lp_bk = T[5], lp_bm_next = T[6],
                    lp_bm_self = T[7], lp_kk = T[8], lp_km = T[9];
        const bool pre_clip = (J.flags & GBX_ABEA_METH_PRE_CLIP) != 0, post_clip = (J.flags & GBX_ABEA_METH_POST_CLIP) != 0;
        // the Gaussian of each of this lane's blocks, scaled to the read (hmm.c:82-92)
        float gm[C], gs[C], gl[C], M[C], B[C], K[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int ki = min(l * C + c, nk - 1);           // blocks past the last k-mer are never updated
            const char *p = J.rc == 0 ? seq + J.seq_off + ki : seq + J.rc_off + (L - ki - GBX_ABEA_KMER);       // hmm.c:382-393
            uint32_t rank = 0;
#pragma unroll
            for (int i = 0; i < GBX_ABEA_KMER; ++i) rank = rank * 5u + meth_rank(p[i]);
            const gbx_abea_model m = model[rank];
            gm[c] = sc * m.level_mean + sh;
            gs[c] = m.level_stdv * vr;
            gl[c] = -0.918938f - (m.level_log_stdv + lv);
            M[c] = B[c] = K[c] = NINF;
        }
        // steps of the wavefront: the longest of its groups
        int steps = have ? rows + nl - 1 : 0;
#pragma unroll
        for (int o = W; o < 64; o <<= 1) steps = max(steps, __shfl_xor(steps, o, 64));
        float pM = NINF, pB = NINF, pK = NINF;               // lane l - 1's last block, the row before
        float lp_end = NINF;
        int rn = min(max(-l, 0), rows - 1);                  // the row of the next step, clamped for the loads
        float x = ev[rn * stride], pre = pre_flank[rn], post = post_flank[rows - 1 - rn];
        for (int t = 0; t < steps; ++t) {
            rn = min(max(t + 1 - l, 0), rows - 1);
            const float xn = ev[rn * stride], pren = pre_flank[rn], postn = post_flank[rows - 1 - rn];
            float cM = __shfl_up(M[C - 1], 1, W), cB = __shfl_up(B[C - 1], 1, W), cK = __shfl_up(K[C - 1], 1, W);
            if (l == 0) cM = cB = cK = NINF;                 // the start block (hmm.c:605-617)
            const int row = t - l;                           // 0-based; the reference's row - 1
            if (have && l < nl && row >= 0 && row < rows) {
                float dM = pM, dB = pB, dK = pK;             // the block to the left, the row before
                float sM = cM, sB = cB, sK = cK;             // the block to the left, this row
                const bool last_row = row == rows - 1;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const int ki = l * C + c;
                    if (ki < nk) {
                        const float a = (x - gm[c]) / gs[c];                                 // hmm.c:59-60
                        const float em = gl[c] + (-0.5f * a * a);
                        float s = lp_mm_self + M[c];                                         // hmm.c:441-456
                        s = meth_logsum(s, lp_mm_next + dM, tbl);
                        s = meth_logsum(s, lp_bm_self + B[c], tbl);
                        s = meth_logsum(s, lp_bm_next + dB, tbl);
                        s = meth_logsum(s, lp_km + dK, tbl);
                        if (c == 0) s = meth_logsum(s, (ki == 0 && (row == 0 || pre_clip)) ? 0.0f + pre : NINF, tbl);
                        const float mn = s + em;
                        const float bn = meth_logsum(lp_mb + M[c], lp_bb + B[c], tbl) + 0.0f;     // hmm.c:459-465
                        float k = meth_logsum(lp_mk + sM, lp_bk + sB, tbl);                  // hmm.c:468-474
                        k = meth_logsum(k, lp_kk + sK, tbl);
                        const float kn = k + 0.0f;
                        dM = M[c]; dB = B[c]; dK = K[c];
                        M[c] = sM = mn; B[c] = sB = bn; K[c] = sK = kn;
                        if (ki == nk - 1 && (post_clip || last_row)) {                       // hmm.c:479-487
                            lp_end = meth_logsum(lp_end, 0.0f + mn + post, tbl);
                            lp_end = meth_logsum(lp_end, 0.0f + bn + post, tbl);
                            lp_end = meth_logsum(lp_end, 0.0f + kn + post, tbl);
                        }
                    }
                }
                pM = cM; pB = cB; pK = cK;
            }
            x = xn; pre = pren; post = postn;
        }
        if (have && l == nl - 1) scores[jid] = lp_end;
    }
}

template <int W, int C>
int meth_launch_class(long long n, const int32_t *d_order, const gbx_abea_meth_job *d_jobs, const char *d_seq, const int64_t *d_event_off,
                      const float *d_event_mean, const float *d_scale, const float *d_shift, const float *d_var, const float *d_log_var,
                      const gbx_abea_model *d_model, const float *d_flogsum, const float *d_trans, const float *d_pre, const float *d_post,
                      float *d_scores, const char *name, hipStream_t s)
{
    if (n <= 0) return GBX_OK;
    const long long tasks = (n + 64 / W - 1) / (64 / W), blocks = (tasks + METH_BLOCK / 64 - 1) / (METH_BLOCK / 64);
    Stage st(name, s);
    hipLaunchKernelGGL((abea_meth_kernel<W, C>), dim3((unsigned)std::min<long long>(blocks, METH_MAX_GRID)), dim3(METH_BLOCK), 0, s, n, d_order,
                       d_jobs, d_seq, d_event_off, d_event_mean, d_scale, d_shift, d_var, d_log_var, d_model, d_flogsum, d_trans, d_pre, d_post,
                       d_scores);
    GBX_HIP(hipGetLastError());
    return GBX_OK;
}

}  // namespace

int abea_meth_launch(int64_t n_jobs, const gbx_abea_meth_job *d_jobs, const char *d_seq, const int64_t *d_event_off, const float *d_event_mean,
                     const float *d_scale, const float *d_shift, const float *d_var, const float *d_log_var, const gbx_abea_model *d_model,
                     const float *d_flogsum, const float *d_trans, const float *d_pre, const float *d_post, const int32_t *d_order,
                     const int64_t *class_off, float *d_scores, hipStream_t s)
{
    if (n_jobs > 0x7fffffffLL - 1024) { set_error("abea meth: more than 2^31 jobs in one call"); return GBX_ERR_UNSUPPORTED; }
    if (class_off[0] != 0 || class_off[GBX_ABEA_METH_NCLASS] != n_jobs) { set_error("abea meth: class_off does not cover the jobs"); return GBX_ERR_ARG; }
    for (int c = 0; c < GBX_ABEA_METH_NCLASS; ++c)
        if (class_off[c + 1] < class_off[c]) { set_error("abea meth: class_off not monotone"); return GBX_ERR_ARG; }
    int rc;
#define METH_CLASS(c, W, C)                                                                                                             \
    if ((rc = meth_launch_class<W, C>(class_off[c + 1] - class_off[c], d_order + class_off[c], d_jobs, d_seq, d_event_off, d_event_mean, \
                                      d_scale, d_shift, d_var, d_log_var, d_model, d_flogsum, d_trans, d_pre, d_post, d_scores,        \
                                      "abea_meth_" #W "x" #C, s)))                                                                      \
        return rc;
    METH_CLASS(0, 16, 1)
    METH_CLASS(1, 64, 1)
    METH_CLASS(2, 64, 2)
    METH_CLASS(3, 64, 4)
#undef METH_CLASS
    return GBX_OK;
}

}  // namespace gbx
