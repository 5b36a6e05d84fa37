/* gbx.h — C-ABI of libgbx.so: MI355X (gfx950) kernels for GenomicsBench's
 * dynamic-programming hot path (bsw, chain, phmm, poa) and its neighbours
 * (abea, fmi, kmer, pileup, dbg).
 *
 * This is the drop-in boundary.  Every entry point is `extern "C"`, takes
 * plain pointers and sizes, returns an int status (0 = GBX_OK, <0 = error;
 * text via gbx_last_error()), never calls exit() and never falls back to a
 * CPU implementation: with no usable HIP device every compute entry point
 * returns GBX_ERR_NO_DEVICE.
 *
 * Two flavours per kernel:
 *   *_host    host buffers in, host buffers out (H2D + kernels + D2H inside;
 *             this is what a reference driver binds to);
 *   *_device  device-resident buffers on a caller-provided hipStream_t (what
 *             bench.py times: inputs already in HBM).
 *
 * Reference interfaces each entry replaces are cited as
 * R/ = /root/reference/ file:line.
 */
#ifndef GBX_H
#define GBX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ status */
#define GBX_OK               0
#define GBX_ERR_ARG         -1   /* bad argument (null pointer, negative size, bad params) */
#define GBX_ERR_NO_DEVICE   -2   /* no HIP device / HIP runtime unusable                   */
#define GBX_ERR_HIP         -3   /* a HIP call failed (see gbx_last_error)                 */
#define GBX_ERR_NOMEM       -4   /* host or device allocation failed                       */
#define GBX_ERR_UNSUPPORTED -5   /* input exceeds a documented limit                       */

const char *gbx_version(void);
const char *gbx_last_error(void);       /* thread-local, never NULL */
int  gbx_device_count(void);            /* number of HIP devices, 0 if none; never errors  */
int  gbx_set_device(int dev);           /* selects the device later calls of this thread use */
int  gbx_device_name(char *buf, size_t cap);
/* Multi-GPU: how many devices of this node the *_host entries spread one call over.  The units of every
 * kernel here are independent, so a call is cut into n contiguous ranges of equal cost (nominal cells / anchors / bases,
 * the same rule as genomicsbench_amd/shard.py), range k runs on device k through a host lane of its own (its own streams,
 * pinned slabs and upload / download threads: the shard goes from the caller's memory straight to that device and its
 * results come back in place) and the call returns when all are done; results are identical to the one-device call.
 * This is the reference's one-engine-per-OpenMP-thread shape (bsw/main_banded.cpp:253-291, chain/src/host_kernel.cpp:98-107,
 * phmm/PairHMMUnitTest.cpp:224-247, poa/msa_spoa_omp.cpp:184-260) with devices in the place of threads.  A call too small
 * to cut (bsw: under 2 x 128 Ki pairs, ...) runs whole on one device and such calls take the devices in turn, so a driver
 * that hands over small slices from many threads still uses every GPU.
 *   n_gpus = 0: the default, i.e. the environment variable GBX_GPUS if set, else 1 (then the calling thread's current
 *   device is used, see gbx_set_device).  Process-wide; not meant to be changed while calls are in flight.
 *   GBX_DEVICE_MAP="0,0,1" (test aid) maps logical devices 0..n-1 onto physical ones: the multi-device path on one GPU.
 * The *_device entries are single-device by construction (the caller owns the buffers and the stream). */
int  gbx_host_set_devices(int n_gpus);
/* The cut itself, for callers that want to see or reuse it: cuts[0..n_parts] with cuts[k] = the first unit index at which the
 * cost of the units before it reaches k / n_parts of the total (negative costs count as 0). */
int  gbx_split_by_cost(int64_t n_units, const double *cost, int n_parts, int64_t *cuts);
int  gbx_host_devices(void);             /* devices the *_host entries currently use (>= 1; 0 without any HIP device) */
/* Optional: creates the calling thread's streams and the pinned staging buffers the *_host entries use for
 * large inputs (about 144 MB of pinned host memory) and runs one small transfer from each buffer on its stream,
 * so that the first large calls do not pay for them.  The
 * counterpart of constructing the reference's aligner object before its timed region
 * (bsw/main_banded.cpp:262-270).  The *_host entries do this themselves on demand. */
int  gbx_host_prepare(void);
/* Optional: puts one device block of `bytes` into the calling thread's lane cache, where the next *_host call
 * that needs a buffer of about that size finds it (e.g. the poa workspace, gbx_poa_workspace_bytes of the plan:
 * ~10 GB for the 'large' job, whose allocation can take seconds right after another process released its
 * memory).  Like gbx_host_prepare this keeps one-time setup out of a caller's timed region. */
int  gbx_host_reserve(size_t bytes);
/* Frees the device memory the *_host entries keep cached between calls (idle lanes only).  Optional. */
int  gbx_host_release(void);
/* Concurrent small calls of gbx_bsw_extend_host / _seqpairs, gbx_phmm_forward_host and gbx_poa_consensus_host are
 * combined: calls that are pending together (the reference drivers' OpenMP threads, one small call each:
 * bsw/main_banded.cpp:279-291, phmm/PairHMMUnitTest.cpp:224-247, poa/msa_spoa_omp.cpp:230-260) share one upload, one launch
 * set and one download, and every caller gets its own results and status.  Nothing to call: GBX_COMBINE=0 in the
 * environment switches it off.  This reads the counters of one kernel (1 bsw, 3 phmm, 4 poa): out[0] calls that were
 * eligible, out[1] device calls made for them, out[2] calls that shared a device call, out[3] most calls in one. */
int  gbx_host_combine_stats(int kernel, uint64_t out[4], int reset);

/* Timing helpers on a stream (HIP events), so that a Python/ctypes host can
 * time the exact stream the kernels are launched on without touching HIP. */
typedef struct gbx_timer gbx_timer;
int  gbx_timer_create(gbx_timer **t);
int  gbx_timer_start(gbx_timer *t, void *stream);
int  gbx_timer_stop(gbx_timer *t, void *stream);
int  gbx_timer_elapsed_ms(gbx_timer *t, float *ms);   /* synchronises on the stop event */
void gbx_timer_destroy(gbx_timer *t);

/* Per-kernel timing: between gbx_profile_begin() and gbx_profile_end() every
 * kernel launched by this thread through a *_device / *_host entry is bracketed
 * by HIP events on its own stream.  gbx_profile_end synchronises and returns,
 * per distinct kernel name (static strings, at most `cap`), the summed
 * duration in ms and the number of launches. */
int  gbx_profile_begin(void);
int  gbx_profile_end(int cap, const char **names, float *ms_sum, int *launches, int *n_stages);

/* Device memory helpers (used by the C++ drivers; bench.py uses torch tensors). */
int  gbx_malloc_device(void **p, size_t bytes);
int  gbx_free_device(void *p);
int  gbx_memcpy_h2d(void *dst, const void *src, size_t bytes, void *stream);
int  gbx_memcpy_d2h(void *dst, const void *src, size_t bytes, void *stream);
int  gbx_stream_synchronize(void *stream);

/* --------------------------------------------------------------------- bsw
 * Banded Smith-Waterman seed extension (bwa-mem2 BSW).
 * Replaces  BandedPairWiseSW::BandedPairWiseSW(...)        R/benchmarks/bsw/bandedSWA.cpp:51-100
 *           BandedPairWiseSW::getScores16(...)              R/benchmarks/bsw/bandedSWA.cpp:1124-1148
 *           (called at R/benchmarks/bsw/main_banded.cpp:286)
 * Per-pair semantics are those of BandedPairWiseSW::scalarBandedSWA
 *           R/benchmarks/bsw/bandedSWA.cpp:128-249 (bwa ksw_extend2), bit-exact.
 */
typedef struct gbx_bsw_params {
    int32_t o_del, e_del, o_ins, e_ins;  /* gap open / extend penalties (>=0; e_* >= 1)   */
    int32_t zdrop;                       /* 100 in the driver, main_banded.cpp:250        */
    int32_t end_bonus;                   /* 5 in the driver                                */
    int32_t w;                           /* band width, 100 in the driver                  */
    int8_t  mat[25];                     /* 5x5 score matrix, bwa_fill_scmat main_banded.cpp:73-81 */
    int8_t  pad_[3];
} gbx_bsw_params;

/* Fills p with the driver's defaults: a=1 b=4 ambig=-1 o=6 e=1 zdrop=100 end_bonus=5 w=100. */
void gbx_bsw_default_params(gbx_bsw_params *p);
/* Same as bwa_fill_scmat(a, b, ambig, mat) (main_banded.cpp:73-81); b is the positive penalty. */
void gbx_bsw_fill_scmat(int a, int b, int ambig, int8_t mat[25]);

/* Per-pair output record, 6 x int32, same field meaning as SeqPair's outputs
 * (R/benchmarks/bsw/bandedSWA.h:91-100). */
typedef struct gbx_bsw_result {
    int32_t score, tle, gtle, qle, gscore, max_off;
} gbx_bsw_result;

/* Mirror of the reference's 72-byte SeqPair (bandedSWA.h:91-100). */
typedef struct gbx_seqpair {
    int64_t idr, idq, id;
    int32_t len1, len2;
    int32_t h0;
    int32_t seqid, regid;
    int32_t score, tle, gtle, qle;
    int32_t gscore, max_off;
} gbx_seqpair;

/* Limits of the device path: query (len2) and target (len1) lengths. */
#define GBX_BSW_MAX_QLEN  8192
#define GBX_BSW_MAX_TLEN  65535

/* Host flat-array entry.  ref/qer are byte arenas of base codes 0..4; pair k's
 * target is ref[idr[k] .. idr[k]+len1[k]), its query qer[idq[k] .. +len2[k]).
 * Writes out[k] for k in [0,n).  Does not write pad records and does not
 * reorder caller memory (cf. bandedSWA.cpp:1172-1177, 1183-1210). */
int gbx_bsw_extend_host(const gbx_bsw_params *p, int64_t n,
                        const uint8_t *ref, int64_t ref_bytes,
                        const uint8_t *qer, int64_t qer_bytes,
                        const int64_t *idr, const int64_t *idq,
                        const int32_t *len1, const int32_t *len2,
                        const int32_t *h0, gbx_bsw_result *out);

/* Drop-in for getScores16 on the reference's own SeqPair array: reads
 * idr/idq/len1/len2/h0 from pairs[k] and writes score,tle,gtle,qle,gscore,
 * max_off in place.  ref_bytes/qer_bytes bound the two arenas. */
int gbx_bsw_extend_seqpairs(const gbx_bsw_params *p, gbx_seqpair *pairs, int64_t n,
                            const uint8_t *ref, int64_t ref_bytes,
                            const uint8_t *qer, int64_t qer_bytes);

/* Device-resident entry: all pointers are device pointers; the arenas must be
 * readable for 16 bytes past their last base (hipMalloc slack is enough);
 * work = scratch of gbx_bsw_workspace_bytes(n) bytes.  Asynchronous on
 * `stream` (a hipStream_t, may be NULL). */
size_t gbx_bsw_workspace_bytes(int64_t n);
int gbx_bsw_extend_device(const gbx_bsw_params *p, int64_t n,
                          const uint8_t *d_ref, const uint8_t *d_qer,
                          const int64_t *d_idr, const int64_t *d_idq,
                          const int32_t *d_len1, const int32_t *d_len2,
                          const int32_t *d_h0, gbx_bsw_result *d_out,
                          void *d_work, size_t work_bytes, void *stream);

/* ------------------------------------------------------------ bsw: seeds
 * Whole-seed extension: bwa-mem2's extension caller (mem_chain2aln: the left extension on the reversed
 * prefixes, then the right one with the left score as its h0, each redone with a doubled band while
 * MAX_BAND_TRY allows, then the local-vs-to-end choice per side).  Every ksw step is the per-pair
 * semantics above (scalarBandedSWA), bit-exact.  For one seed, with a = mat[0] and ksw(Q, T, h0, w, bonus):
 *
 *   score = truesc = -1; aw0 = aw1 = w
 *   if qbeg > 0:      Q = reverse(read[0:qbeg]), T = reverse(win[0:rbeg]), h0 = len*a, bonus = pen_clip5
 *                     try i = 0..max_band_try-1 with band aw0 = w << i; stop when the score did not change or
 *                     max_off < aw0/2 + aw0/4;  local (qb = qbeg-qle, rb = rbeg-tle, truesc = score) unless
 *                     gscore > 0 and gscore > score - pen_clip5: to-end (qb = 0, rb = rbeg-gtle, truesc = gscore)
 *   else:             score = truesc = len*a, qb = 0, rb = rbeg
 *   sc0 = score
 *   if qbeg+len < lq: Q = read[qbeg+len:lq], T = win[rbeg+len:rlen], h0 = sc0, bonus = pen_clip3, tries as above
 *                     (the first try's "previous score" is sc0); local qe = q0+qle, re = r0+tle, truesc += score-sc0,
 *                     or to-end qe = lq, re = r0+gtle, truesc += gscore-sc0
 *   else:             qe = lq, re = rbeg+len
 *   w_out = max(aw0, aw1)
 *
 * Coordinates are half-open; rb/re are relative to the seed's window (bwa adds rmax[0]).  Chaining, seedcov
 * and the choice of seeds stay with the caller.
 */
typedef struct gbx_bsw_seed_params {
    gbx_bsw_params bsw;              /* scoring, zdrop, w; bsw.end_bonus is not read                       */
    int32_t pen_clip5, pen_clip3;    /* end bonus of the left / right extension (bwa: 5 / 5)               */
    int32_t max_band_try;            /* 1..4; bwa's MAX_BAND_TRY is 2                                      */
    int32_t pad_;
} gbx_bsw_seed_params;

/* gbx_bsw_default_params with pen_clip5 = pen_clip3 = 5, max_band_try = 2 (bwa mem's defaults). */
void gbx_bsw_seed_default_params(gbx_bsw_seed_params *p);

/* One seed: the read is qer[qoff .. qoff+lq), its reference window ref[roff .. roff+rlen), and the exact
 * match read[qbeg, qbeg+len) ~ win[rbeg, rbeg+len) (not checked).  Rules: 0 <= qbeg, 1 <= len,
 * qbeg+len <= lq, 0 <= rbeg, rbeg+len <= rlen, both ranges inside their arenas; the left side (qbeg x rbeg)
 * and the right side (lq-qbeg-len x rlen-rbeg-len) within GBX_BSW_MAX_QLEN x GBX_BSW_MAX_TLEN. */
typedef struct gbx_bsw_seed {        /* 40 bytes */
    int64_t qoff, roff;
    int32_t lq, rlen, qbeg, rbeg, len, pad_;
} gbx_bsw_seed;

typedef struct gbx_bsw_seed_result { /* 32 bytes */
    int32_t score, truesc, qb, qe, rb, re, w;
    int32_t sc0;                     /* the h0 handed to the right extension */
} gbx_bsw_seed_result;

/* Host buffers in and out.  All seeds and parameters are checked before any device is touched: a bad seed
 * gives GBX_ERR_ARG (GBX_ERR_UNSUPPORTED past the length limits) naming the lowest such seed. */
int gbx_bsw_extend_seeds_host(const gbx_bsw_seed_params *p, int64_t n,
                              const uint8_t *ref, int64_t ref_bytes, const uint8_t *qer, int64_t qer_bytes,
                              const gbx_bsw_seed *seeds, gbx_bsw_seed_result *out);

/* Device entry: all pointers are device pointers, the arenas readable for 16 bytes past their end (hipMalloc
 * slack is enough); work = scratch of gbx_bsw_seeds_workspace_bytes(n, ref_bytes, qer_bytes) bytes.
 * Asynchronous on `stream`: no host synchronisation between the phases.  The seeds are on the device and are
 * not checked on the host; a seed that breaks the rules gets a result of all -1 and is not extended. */
size_t gbx_bsw_seeds_workspace_bytes(int64_t n, int64_t ref_bytes, int64_t qer_bytes);
int gbx_bsw_extend_seeds_device(const gbx_bsw_seed_params *p, int64_t n,
                                const uint8_t *d_ref, int64_t ref_bytes, const uint8_t *d_qer, int64_t qer_bytes,
                                const gbx_bsw_seed *d_seeds, gbx_bsw_seed_result *d_out,
                                void *d_work, size_t work_bytes, void *stream);

/* ------------------------------------------------------------------- chain
 * minimap2 anchor chaining DP.
 * Replaces  host_chain_kernel(std::vector<call_t>&, std::vector<return_t>&, int)
 *           R/benchmarks/chain/src/host_kernel.cpp:96-108  (chain_dp :30-94)
 * Calls are concatenated: call c owns anchors [anchor_off[c], anchor_off[c+1]).
 */
typedef struct gbx_chain_call {
    float   avg_qspan;                         /* host_data.h:24-29 */
    int32_t max_dist_x, max_dist_y, bw, n_segs;
} gbx_chain_call;

#define GBX_CHAIN_MAX_ITER 5000   /* host_kernel.cpp:37 */
#define GBX_CHAIN_MAX_SKIP 25     /* host_kernel.cpp:38 */

/* target/peak may be NULL (the reference computes them but never prints them). */
int gbx_chain_host(int64_t n_calls, const int64_t *anchor_off,
                   const uint64_t *ax, const uint64_t *ay,
                   const gbx_chain_call *hdr,
                   int32_t *score, int32_t *parent,
                   int32_t *target, int32_t *peak);

size_t gbx_chain_workspace_bytes(int64_t n_calls, int64_t n_anchors);
int gbx_chain_device(int64_t n_calls, int64_t n_anchors, const int64_t *d_anchor_off,
                     const uint64_t *d_ax, const uint64_t *d_ay,
                     const gbx_chain_call *d_hdr,
                     int32_t *d_score, int32_t *d_parent,
                     int32_t *d_target, int32_t *d_peak,
                     void *d_work, size_t work_bytes, void *stream);

/* Work counter of the last gbx_chain_device call on this workspace: predecessor pairs (i,j) visited,
 * `continue`d ones included, those after the max_skip break excluded (the benchmark's "cell"). */
int gbx_chain_evaluated_pairs(const void *d_work, int64_t *pairs, void *stream);

/* How the last gbx_chain_device call on this workspace was scheduled: a call whose anchors are sorted by x falls apart
 * at every anchor that lies further than max_dist_x behind its predecessor (it looks back at nobody and nothing later
 * looks across it, host_kernel.cpp:56) into pieces that are chained independently (`jobs` >= calls; at most one cut per
 * 64 anchors); `longest_job` = anchors of the longest piece, what bounds the kernel's makespan. */
int gbx_chain_job_stats(const void *d_work, int64_t n_calls, int64_t n_anchors, int64_t *jobs, int64_t *longest_job, void *stream);

/* -------------------------------------------------------------------- phmm
 * GATK/GKL Pair-HMM forward log10-likelihoods.
 * Replaces  void initPairHMM()                                     R/benchmarks/phmm/PairHMMUnitTest.cpp:84,193
 *           void computelikelihoodsboth(testcase*, double*, int)   R/benchmarks/phmm/PairHMMUnitTest.cpp:86,245
 *           (C++-mangled symbols of libgkl_pairhmm_c.so; `testcase` = pairhmm_common.h:20-24)
 * Reads live in one arena per track (bases rs and the four quality tracks q,i,d,c share
 * read_off/read_len; qualities already Phred-33 as the driver normalises them,
 * PairHMMUnitTest.cpp:89-93,110-113), haplotypes in another; pair p = (read pair_read[p],
 * haplotype pair_hap[p]).  out[p] = log10 likelihood (fp32 pass, fp64 redo below 1e-28f,
 * pairhmm_common.h:16).  Tolerance vs the CPU path: 1e-5 relative.
 */
#define GBX_PHMM_MAX_HAPLEN 32768     /* MAX_HAP_LENGTH, PairHMMUnitTest.h:36 */

int gbx_phmm_init(void);              /* builds + uploads the probability tables (initPairHMM) */

int gbx_phmm_forward_host(int64_t n_pairs, const int32_t *pair_read, const int32_t *pair_hap,
                          int64_t n_reads, const int64_t *read_off, const int32_t *read_len, int64_t read_bytes,
                          const uint8_t *rs, const uint8_t *q, const uint8_t *i, const uint8_t *d, const uint8_t *c,
                          int64_t n_haps, const int64_t *hap_off, const int32_t *hap_len, int64_t hap_bytes,
                          const uint8_t *hap, double *out);

/* The device entry groups the pairs by read (workspace arrays indexed by read id, hence n_reads) and
 * materialises one haplotype byte stream per read: workspace ~ n_pairs * (max_hap_len + 1) bytes.
 * The haplotype arena must be readable for 16 bytes past its last base (hipMalloc slack is enough). */
size_t gbx_phmm_workspace_bytes(int64_t n_pairs, int64_t n_reads, int32_t max_hap_len);
int gbx_phmm_forward_device(int64_t n_pairs, const int32_t *d_pair_read, const int32_t *d_pair_hap,
                            int64_t n_reads, const int64_t *d_read_off, const int32_t *d_read_len,
                            const uint8_t *d_rs, const uint8_t *d_q, const uint8_t *d_i, const uint8_t *d_d,
                            const uint8_t *d_c,
                            const int64_t *d_hap_off, const int32_t *d_hap_len, const uint8_t *d_hap,
                            int32_t max_hap_len, double *d_out,
                            void *d_work, size_t work_bytes, void *stream);

/* --------------------------------------------------------------------- poa
 * Partial-order-alignment consensus (spoa).
 * Replaces, at whole-window granularity, the driver's per-window loop
 *   spoa::createAlignmentEngine(kNW, m, n, g, e, q, c)   R/benchmarks/poa/msa_spoa_omp.cpp:189-190
 *   spoa::createGraph()                                   :237
 *   AlignmentEngine::align(seq, graph)                    :242
 *   Graph::add_alignment(alignment, seq)                  :247
 *   Graph::generate_consensus()                           :252
 * Window w owns sequences [win_first_seq[w], win_first_seq[w+1]); sequence s is
 * arena[seq_off[s] .. seq_off[s]+seq_len[s]).
 */
typedef struct gbx_poa_params {
    int8_t m, n;      /* match score (2) and mismatch score (-4), msa_spoa_omp.cpp:157-158 */
    int8_t g, e;      /* first gap piece: open(-6 = o1+e1) / extend(-2), :184 */
    int8_t q, c;      /* second gap piece: open(-25 = o2+e2) / extend(-1) */
    int8_t pad_[2];
} gbx_poa_params;

void gbx_poa_default_params(gbx_poa_params *p);

/* Capacities of the device path for a set of windows (computed from host metadata). */
typedef struct gbx_poa_plan {
    int32_t max_seq_len;          /* longest sequence                                    */
    int32_t max_seqs_per_window;  /* bounds the fan-in / fan-out of a graph node          */
    int32_t node_cap;             /* graph nodes per window the workspace can hold       */
    int32_t n_slots;              /* windows processed concurrently (one wavefront each) */
    /* Windows that hold a sequence of more than 512 bases run on a second launch with slots of their own (five int16
     * planes per DP matrix instead of two): a handful of long sequences must not size every slot of the job. */
    int32_t n_long_windows;       /* windows with a sequence longer than 512             */
    int32_t long_slots;           /* slots of the second launch (0 when there is none)   */
    int64_t n_windows;            /* windows the plan was made for                       */
} gbx_poa_plan;

#define GBX_POA_MAX_SEQS_PER_WINDOW 255
#define GBX_POA_MAX_LETTERS_PER_COLUMN 8

/* per-window status bits written by the device path (0 = ok) */
#define GBX_POA_ST_NODES   1   /* node_cap exceeded                      */
#define GBX_POA_ST_DEGREE  2   /* fan-in/out above max_seqs_per_window   */
#define GBX_POA_ST_LETTERS 4   /* more than 8 distinct letters aligned   */
#define GBX_POA_ST_STACK   8
#define GBX_POA_ST_CONS    16  /* consensus longer than cons_stride      */

int gbx_poa_plan_host(int64_t n_windows, const int64_t *win_first_seq, const int32_t *seq_len, gbx_poa_plan *plan);
size_t gbx_poa_workspace_bytes(const gbx_poa_plan *plan);

/* DP cells of the last gbx_poa_consensus_device call on this workspace: sum over alignments of
 * graph nodes x sequence length. */
int gbx_poa_cells(const gbx_poa_plan *plan, const void *d_work, int64_t *cells, void *stream);

/* cons: n_windows rows of cons_stride bytes (not NUL-terminated), cons_len[w] = consensus length.
 * Returns GBX_ERR_UNSUPPORTED (and names the first window) if any window overflowed a capacity. */
int gbx_poa_consensus_host(const gbx_poa_params *p, int64_t n_windows, const int64_t *win_first_seq,
                           int64_t n_seqs, const int64_t *seq_off, const int32_t *seq_len,
                           const char *arena, int64_t arena_bytes,
                           char *cons, int32_t *cons_len, int64_t cons_stride);

/* Device-resident entry; d_status[w] receives the GBX_POA_ST_* bits. */
int gbx_poa_consensus_device(const gbx_poa_params *p, const gbx_poa_plan *plan, int64_t n_windows,
                             const int64_t *d_win_first_seq, const int64_t *d_seq_off, const int32_t *d_seq_len,
                             const char *d_arena, char *d_cons, int32_t *d_cons_len, int32_t *d_status,
                             int64_t cons_stride, void *d_work, size_t work_bytes, void *stream);

/* -------------------------------------------------------------------- abea
 * Adaptive banded event alignment of nanopore events to the k-mers of a read's basecalled sequence (f5c /
 * nanopolish; SURVEY §8f rank 4: the suite's other banded DP).
 * Replaces  int32_t align(AlignedPair *out, char *sequence, int32_t sequence_len, event_table events,
 *                         model_t *models, scalings_t scaling, float sample_rate)
 *           R/benchmarks/abea/src/align.c:169-548, called per read by align_single, f5c.c:1344-1349
 *           (the suite's CUDA path for the same step: align.cu:140-560 - not a template for this code).
 * Semantics are those of the CPU function, bit for bit: float band scores and emissions, double transition
 * penalties (every candidate is a double sum rounded to float), Suzuki's adaptive band placement, the traceback,
 * the double emission sum and the three QC rules that empty an alignment.  `sample_rate` is unused by align()
 * (:108-126) and has no counterpart here.  Of an event only its mean is read (:125).
 */
#define GBX_ABEA_BANDWIDTH 100     /* ALN_BANDWIDTH, f5c.h:28 */
#define GBX_ABEA_KMER      6       /* KMER_SIZE, f5c.h:24 */
#define GBX_ABEA_NMODEL    4096    /* 4^KMER_SIZE model states */

typedef struct gbx_abea_model {   /* model_t with CACHED_LOG, f5c.h:122-136 */
    float level_mean, level_stdv, level_log_stdv;     /* level_log_stdv = log(level_stdv), model.c:53 */
} gbx_abea_model;
typedef struct gbx_abea_event {   /* event_t, f5c.h:104-111 (24 bytes) */
    uint64_t start;
    float length, mean, stdv;
} gbx_abea_event;
typedef struct gbx_abea_pair {    /* AlignedPair, f5c.h:163-166 */
    int32_t ref_pos, read_pos;    /* k-mer index, event index */
} gbx_abea_pair;

/* Read r: bases seq_arena[seq_off[r] .. +seq_len[r]) (A/C/G/T; anything else ranks as A, align.c:10-24), events
 * [event_off[r], event_off[r+1]) of the concatenated event array, scalings scale[r], shift[r] (scalings_t, f5c.h:139-155).
 * Output: pairs of read r at out + 2*event_off[r] (the reference sizes the array 2 x n_events, f5c.c), n_pairs[r] of
 * them in ascending order, 0 when a QC rule failed (align.c:530-541); the slots of a read behind its n_pairs are
 * unspecified.  seq_len >= KMER and >= 1 event per read. */
int gbx_abea_align_host(int64_t n_reads, const int64_t *seq_off, const int32_t *seq_len, const char *seq_arena,
                        int64_t seq_bytes, const int64_t *event_off, const gbx_abea_event *events,
                        const gbx_abea_model *models, const float *scale, const float *shift,
                        gbx_abea_pair *out, int32_t *n_pairs);

/* Device path.  gbx_abea_plan_host computes from host metadata the per-read offsets into the band workspace
 * (band_off[n_reads+1], in bands), the processing order (longest first) and the two read-dependent transition
 * penalties, which are double logarithms (align.c:195-204) and are taken with the host C library so that they are the
 * reference's bits; the device entry takes the compact float array of event means.  n_kmers_total = sum of
 * seq_len - KMER + 1, n_bands_total = band_off[n_reads].
 * Indexing of the device entry: ABSOLUTE - read r's means are d_event_mean[d_event_off[r] ..], its pairs are written at
 * d_out + 2*d_event_off[r]; d_event_off[0] need not be 0 (both arrays must then reach up to d_event_off[n_reads]). */
int gbx_abea_plan_host(int64_t n_reads, const int32_t *seq_len, const int64_t *event_off,
                       int64_t *band_off, int32_t *order, double *lp /* [n_reads][2]: lp_stay, lp_step, align.c:195-204 */);
size_t gbx_abea_workspace_bytes(int64_t n_reads, int64_t n_kmers_total, int64_t n_bands_total);
int gbx_abea_align_device(int64_t n_reads, const int64_t *d_seq_off, const int32_t *d_seq_len, const char *d_seq_arena,
                          const int64_t *d_event_off, const float *d_event_mean, const gbx_abea_model *d_models,
                          const float *d_scale, const float *d_shift, const int64_t *d_band_off, const int32_t *d_order,
                          const double *d_lp, int64_t n_kmers_total, int64_t n_bands_total,
                          gbx_abea_pair *d_out, int32_t *d_n_pairs, void *d_work, size_t work_bytes, void *stream);
/* DP cells filled by the last gbx_abea_align_device call on this workspace (the reference's `fills`, align.c:280,401). */
int gbx_abea_cells(const void *d_work, int64_t *cells, void *stream);

/* abea from raw signal: what f5c runs per read before align() (event_single, f5c.c:1219-1242): ADC counts -> pA
 * (f5c.c:1227-1231), scrappie's event detection (detect_events, events.c:292-549, the DNA defaults: windows 3 / 6,
 * thresholds 1.4 / 9.0, peak height 0.2; getevents() discards the result of its MAD trimming, so detection runs over
 * all samples) and estimate_scalings_using_mom (align.c:49-97).  Bit for bit the reference's order of operations.
 * Read r: samples raw[raw_off[r] .. raw_off[r+1]) of one int16 arena, pA = ((float)adc + offset[r]) * (range[r] /
 * digitisation[r]).  Output: n_events[r] records at events + event_off[r] (event_off[n_reads] = their total) and the
 * compact means beside them - the layout gbx_abea_align_device reads.
 * The one deviation: the reference is undefined for a read in which no peak is found (it reads peaks[-1]; fewer than
 * 12 samples, no sample, constant signal).  Such a read has n_events = 0 and GBX_ABEA_EV_NONE in its status, scale =
 * shift = 0, and the chained entry reports n_pairs = 0 for it.  Single device only. */
#define GBX_ABEA_EV_NONE     1    /* status: no peak found, the read has no events                               */
#define GBX_ABEA_EV_INORDER  2    /* status: the cumulative sums were taken in index order (the read fails the    */
                                  /* exactness predicate of DESIGN 3.5), not by the wavefront scan                */
#define GBX_ABEA_EV_OVERFLOW 4    /* status: the fill pass left the read's events unwritten (past event_cap)      */
#define GBX_ABEA_EVENTS_COUNT 1   /* pass: n_events, event_off and status from the signal                         */
#define GBX_ABEA_EVENTS_FILL  2   /* pass: events and means at the event_off of a count pass                      */

/* Device entry.  pass = COUNT: writes d_n_events[n_reads], d_event_off[n_reads + 1], d_status[n_reads] (d_events and
 * d_event_mean may be NULL).  pass = FILL: reads d_event_off and d_status of a count pass over the same input and writes
 * the records; a read whose events would end past event_cap is left unwritten and flagged.  COUNT | FILL does both
 * (the caller then sizes the two arrays by a bound of its own).  Nothing is synchronised. */
int gbx_abea_events_device(int pass, int64_t n_reads, const int16_t *d_raw, const int64_t *d_raw_off, const float *d_range,
                           const float *d_digitisation, const float *d_offset, int64_t *d_n_events, int64_t *d_event_off,
                           gbx_abea_event *d_events, float *d_event_mean, int64_t event_cap, int32_t *d_status, void *stream);
/* scale[r], shift[r] from the read's event means and the model levels of its k-mers; event_off as above (absolute). */
int gbx_abea_scalings_device(int64_t n_reads, const int64_t *d_seq_off, const int32_t *d_seq_len, const char *d_seq_arena,
                             const int64_t *d_event_off, const float *d_event_mean, const gbx_abea_model *d_models,
                             float *d_scale, float *d_shift, void *stream);
/* Host-buffer entries.  event_cap = the records `events` has room for; *n_events_total = the number found.  More than
 * event_cap gives GBX_ERR_ARG with the needed count in *n_events_total and gbx_last_error(); n_events, event_off and
 * status are valid then, events (and everything behind them) are not. */
int gbx_abea_events_host(int64_t n_reads, const int16_t *raw, const int64_t *raw_off, const float *range,
                         const float *digitisation, const float *offset, int64_t *n_events, int64_t *event_off,
                         gbx_abea_event *events, int64_t event_cap, int64_t *n_events_total, int32_t *status);
/* raw signal -> events -> scalings -> align on one device.  out holds 2 * event_cap pairs, read r's at out +
 * 2 * event_off[r] as in gbx_abea_align_host; seq_len >= KMER for every read. */
int gbx_abea_signal_align_host(int64_t n_reads, const int16_t *raw, const int64_t *raw_off, const float *range,
                               const float *digitisation, const float *offset, const int64_t *seq_off, const int32_t *seq_len,
                               const char *seq_arena, int64_t seq_bytes, const gbx_abea_model *models, int64_t *event_off,
                               gbx_abea_event *events, int64_t event_cap, int64_t *n_events_total, float *scale, float *shift,
                               int32_t *status, gbx_abea_pair *out, int32_t *n_pairs);

/* abea, methylation scoring: what f5c call-methylation runs per read behind align() (meth_single, f5c.c:1375-1380).
 * Replaces  float profile_hmm_score(m_seq, m_rc_seq, event, scaling, cpgmodel, event_start_idx, event_stop_idx, strand,
 *                                   event_stride, rc, events_per_base, hmm_flags)            hmm.c:301-727
 *           void  calculate_methylation_for_read(site_score_map, ref, record, ...)           meth.c:500-658 (the planner)
 * A job is one profile_hmm_score call: the forward score of a run of events under a sequence over A/C/G/M/T, three
 * states per k-mer, every log-sum the table-driven p7_FLogsum (ESL_LOG_SUM, f5c.h:70; logsum.h:61-71).  The score is the
 * CPU function's, bit for bit: the six candidates of a cell folded left to right, lp_end accumulated in row order, the
 * float emission with its division (hmm.c:55-100).  HMM_REVERSE_FIX is not defined: with rc the k-mers are read from the
 * reverse-complement string backwards and the events are walked downwards (hmm.c:382-393, 429).  A base outside ACGMT
 * ranks as A.  Reads with events_per_base <= 1 give an unspecified score. */
#define GBX_ABEA_NMODEL_CPG      15625   /* 5^KMER_SIZE states, A < C < G < M < T (hmm.c:21-52) */
#define GBX_ABEA_FLOGSUM_TBL     16000   /* p7_LOGSUM_TBL, logsum.h:18 */
#define GBX_ABEA_METH_PRE_CLIP   1       /* HAF_ALLOW_PRE_CLIP, f5cmisc.h:15 */
#define GBX_ABEA_METH_POST_CLIP  2       /* HAF_ALLOW_POST_CLIP */
#define GBX_ABEA_METH_NTRANS     10      /* per read: lp_mk mb mm_self mm_next bb bk bm_next bm_self kk km (hmm.c:212-229) */
#define GBX_ABEA_METH_MAX_KMERS  256     /* k-mers of one job; the planner's span rule keeps a group at 216 (meth.c:571) */
#define GBX_ABEA_METH_NCLASS     4       /* kernel classes by k-mer count: <= 16, <= 64, <= 128, <= 256 */

typedef struct gbx_abea_meth_job {
    int64_t seq_off, rc_off;          /* m_seq and m_rc_seq in the string arena, seq_len bytes each */
    int32_t seq_len;                  /* >= KMER */
    int32_t read;                     /* the read whose events, scalings and transitions it uses */
    int32_t event_start, event_stop;  /* event_start_idx, event_stop_idx: indices into the read's own events, inclusive */
    int32_t rc;                       /* event_stride = -1 iff rc (hmm.c:322): event_stop <= event_start then */
    int32_t flags;                    /* GBX_ABEA_METH_PRE_CLIP | GBX_ABEA_METH_POST_CLIP */
} gbx_abea_meth_job;
typedef struct gbx_abea_meth_site {   /* ScoredSite, f5c.h:193-218, without the scores: job 2s is the unmethylated, 2s+1 the methylated */
    int32_t read, start_position, end_position, n_cpg;
    int64_t ctx_off;                  /* ScoredSite::sequence = the disambiguated reference segment of the read at */
    int32_t ctx_len, pad_;            /* [ctx_off, ctx_off + ctx_len) */
} gbx_abea_meth_site;

/* Everything that needs the host C library, so that it carries the reference's bits: the p7_FLogsum table (logsum.h:44-46),
 * the transition logs of every read (hmm.c:247-295; float logarithms: the reference is compiled as C++, where log of a
 * float is the float overload), the two flank tables (flank_len entries each, flank_len > the largest row count of the
 * batch; pre_flank[i] as hmm.c:172-205, post_flank[j] = the reference's post_flank[n_events - 1 - j], hmm.c:132-168) and
 * the processing order: jobs by kernel class, longest first within a class; class_off[c] .. class_off[c + 1] of `order`
 * are class c's.  Checks every job against the arena, its read's events and GBX_ABEA_METH_MAX_KMERS. */
int gbx_abea_meth_plan_host(int64_t n_jobs, const gbx_abea_meth_job *jobs, int64_t seq_bytes, int64_t n_reads,
                            const int64_t *event_off, const double *events_per_base, float *flogsum, float *trans,
                            int64_t flank_len, float *pre_flank, float *post_flank, int32_t *order,
                            int64_t *class_off /* [GBX_ABEA_METH_NCLASS + 1] */);
/* Device entry: d_scores[j] = the score of job j.  Jobs, strings, reads, plan and model resident in device memory;
 * class_off is the plan's, on the host.  d_event_off indexes d_event_mean ABSOLUTELY as in gbx_abea_align_device.  No
 * workspace; nothing is synchronised. */
int gbx_abea_meth_score_device(int64_t n_jobs, const gbx_abea_meth_job *d_jobs, const char *d_seq_arena,
                               const int64_t *d_event_off, const float *d_event_mean, const float *d_scale, const float *d_shift,
                               const float *d_var, const float *d_log_var, const gbx_abea_model *d_cpg_model,
                               const float *d_flogsum, const float *d_trans, const float *d_pre_flank, const float *d_post_flank,
                               const int32_t *d_order, const int64_t *class_off, float *d_scores, void *stream);
/* Pageable host buffers in, scores out (one device).  events: the 24-byte records, read r's at events + event_off[r]. */
int gbx_abea_meth_score_host(int64_t n_jobs, const gbx_abea_meth_job *jobs, const char *seq_arena, int64_t seq_bytes,
                             int64_t n_reads, const int64_t *event_off, const gbx_abea_event *events, const float *scale,
                             const float *shift, const float *var, const float *log_var, const double *events_per_base,
                             const gbx_abea_model *cpg_model, float *scores);
/* sum over the jobs of rows x k-mers x 3 states */
int gbx_abea_meth_cells(int64_t n_jobs, const gbx_abea_meth_job *jobs, int64_t *cells);
/* The site planner: calculate_methylation_for_read without the BAM record.  Read r: reference segment ref_arena[ref_off[r]
 * .. +ref_len[r]) (any case, IUPAC codes; disambiguated as meth.c:288-306), ref_start_pos[r], rc[r], and its
 * event-alignment record rec[rec_off[r] .. rec_off[r + 1]): (ref_pos, event_idx) sorted by ref_pos, what
 * get_event_alignment_record returns (meth.c:124-185).  Writes *n_sites sites, 2 * *n_sites jobs (flags 3) and their four
 * strings each into seq_arena (*seq_bytes bytes).  Reproduces the CpG scan and grouping at min_separation 10, the skips
 * sub_start_pos <= 10 and span > 200, find_by_ref_bounds, the |e2 - e1| <= 10 filter and the ratio filter as written (it
 * divides by a negative number and never rejects).  More sites than site_cap or more bytes than seq_cap: GBX_ERR_ARG with
 * the needed counts in *n_sites and *seq_bytes (call with 0 / NULL to size).  A record that runs against rc (the reference
 * asserts, hmm.c:322) is GBX_ERR_ARG. */
int gbx_abea_meth_sites_host(int64_t n_reads, const int64_t *ref_off, const int32_t *ref_len, const char *ref_arena,
                             const int32_t *ref_start_pos, const uint8_t *rc, const int64_t *rec_off, const gbx_abea_pair *rec,
                             int64_t site_cap, gbx_abea_meth_site *sites, gbx_abea_meth_job *jobs, int64_t *n_sites,
                             int64_t seq_cap, char *seq_arena, int64_t *seq_bytes);
/* The site planner on the device, behind gbx_abea_event_record_device: the inputs of gbx_abea_meth_sites_host resident in
 * device memory, the output byte for byte the host planner's.  pass COUNT writes d_site_off[n_reads + 1] and
 * d_byte_off[n_reads + 1] (exclusive scans, the totals in entry n_reads) and d_bad[r] = 1 for a read whose record runs
 * against rc[r] (the host planner refuses the batch; what such a read counts means nothing).  pass FILL writes, at the offsets of a count pass,
 * the sites, 2 * n_sites jobs and the strings; a read whose sites would end past site_cap or whose strings would end past
 * seq_cap is left unwritten.  d_work: gbx_abea_meth_sites_work bytes (ref_bytes, the bytes of the reference arena, does not
 * enter it today: a closed group is decided in registers).  A record longer than 2^31 - 1 pairs is read that far.  Nothing
 * is synchronised. */
#define GBX_ABEA_METH_SITES_COUNT 1
#define GBX_ABEA_METH_SITES_FILL  2
int64_t gbx_abea_meth_sites_work(int64_t n_reads, int64_t ref_bytes);
int gbx_abea_meth_sites_device(int pass, int64_t n_reads, const int64_t *d_ref_off, const int32_t *d_ref_len,
                               const char *d_ref_arena, const int32_t *d_ref_start_pos, const uint8_t *d_rc,
                               const int64_t *d_rec_off, const gbx_abea_pair *d_rec, void *d_work, int64_t *d_site_off,
                               int64_t *d_byte_off, uint8_t *d_bad, int64_t site_cap, gbx_abea_meth_site *d_sites,
                               gbx_abea_meth_job *d_jobs, int64_t seq_cap, char *d_seq_arena, void *stream);
/* The half of gbx_abea_meth_plan_host that needs the host C library: the p7_FLogsum table, trans[n_reads][NTRANS] and the
 * two flank tables, in its bits.  gbx_abea_meth_plan_host calls it. */
int gbx_abea_meth_tables_host(int64_t n_reads, const double *events_per_base, float *flogsum, float *trans, int64_t flank_len,
                              float *pre_flank, float *post_flank);
/* The other half on the device: d_order[n_jobs] and d_class_off[GBX_ABEA_METH_NCLASS + 1] as gbx_abea_meth_plan_host gives
 * them (class by k-mer count, longest first, ties in input order), and its per-job checks: *d_first_bad (device int64) is
 * the lowest job that gbx_abea_meth_plan_host would refuse, INT64_MAX when there is none.  The score kernel indexes events
 * with what the jobs say: read d_class_off and d_first_bad back, and do not launch the score when a job is bad.
 * max_rows_bits (1 .. 30): the sort key's bits for the row count; flank_len <= 2^max_rows_bits.  d_work:
 * gbx_abea_meth_order_work bytes.  Nothing is synchronised. */
int64_t gbx_abea_meth_order_work(int64_t n_jobs);
int gbx_abea_meth_order_device(int64_t n_jobs, const gbx_abea_meth_job *d_jobs, int64_t seq_bytes, int64_t n_reads,
                               const int64_t *d_event_off, int64_t flank_len, int max_rows_bits, void *d_work,
                               int32_t *d_order, int64_t *d_class_off, int64_t *d_first_bad, void *stream);
/* The TSV f5c call-methylation prints (f5c.c:1629-1653; with_header: the header of meth_main.c:449-457 first).  Site s
 * with scores[2 s] unmethylated and scores[2 s + 1] methylated: contig, (version 2: strand,) start, end, read name, the
 * difference of the two scores as doubles, both scores ("%.2lf"), strands_scored 1, n_cpg and the context, ctx_len bytes at
 * ctx_off of the read's disambiguated reference segment.  A site is printed unless (clip_start != -1 && start_position <
 * clip_start) || (clip_end != -1 && end_position >= clip_end).  *n_bytes: the bytes of text; more than cap: GBX_ERR_ARG
 * with the need in *n_bytes (call with 0 / NULL to size). */
int gbx_abea_meth_tsv_host(int64_t n_sites, const gbx_abea_meth_site *sites, const float *scores, int64_t n_reads,
                           const char *const *read_names, const char *const *contig_names, const uint8_t *rc,
                           const int64_t *ref_off, const int32_t *ref_len, const char *ref_arena, int version, int32_t clip_start,
                           int32_t clip_end, int with_header, int64_t cap, char *out, int64_t *n_bytes);

/* abea, methylation frequency: f5c meth-freq (freq.c), the stage behind call-methylation that folds the per-read calls into one
 * line per genomic site.  Replaces  int freq_main(int argc, char **argv)   freq.c:253-430.
 * A record is one line of the call-methylation TSV: contig (the rank of its name among the run's names under strcmp), start,
 * end, n_cpg, llr (log_lik_ratio as meth-freq reads it: strtod of the printed text) and the sequence, seq_len bytes at seq_off
 * of an arena.  A record with fabs(llr) < threshold is dropped (so NaN is kept); it is methylated iff llr > 0.  Without
 * split_groups, or when n_cpg <= 1, it is one item of weight n_cpg under the key (contig, start, end); otherwise one item of
 * weight 1 per occurrence of "CG" in its sequence, at start + pos - first_pos for both start and end, with the sequence
 * "split-group".  Per key: called_sites and called_sites_methylated are the sums of the weights; group_size and the sequence
 * are those of the first item in input order.  Keys with called_sites == 0 are not in the table.  The table is sorted by
 * contig, start, end; a site's sequence is seq_len bytes at seq_off of the arena the table owns, seq_len == -1 is "split-group".
 * Limits: a sum above INT32_MAX (the reference's int overflows) and a split position above INT32_MAX are GBX_ERR_UNSUPPORTED. */
typedef struct gbx_abea_freq_record {
    int32_t contig, start, end, n_cpg;
    double  llr;
    int64_t seq_off;
    int32_t seq_len, pad_;
} gbx_abea_freq_record;
typedef struct gbx_abea_freq_site {
    int32_t contig, start, end, group_size, called_sites, called_sites_methylated;
    int64_t seq_off;
    int32_t seq_len, pad_;             /* seq_len == -1: "split-group" (seq_off 0) */
} gbx_abea_freq_site;
#define GBX_ABEA_FREQ_COUNT   1        /* pass: the per-record item counts and their offsets */
#define GBX_ABEA_FREQ_REDUCE  2        /* pass: items, sort, segments, sums; the table's sizes */
#define GBX_ABEA_FREQ_FILL    4        /* pass: the table and its arena */
#define GBX_ABEA_FREQ_NCOUNTS 8        /* d_counts: int64 [0] items [1] keys [2] sites [3] arena bytes [4] flags */
#define GBX_ABEA_FREQ_SUM_OVERFLOW 1   /* flags: a site's sum is above INT32_MAX */
#define GBX_ABEA_FREQ_POS_OVERFLOW 2   /*        a split position is above INT32_MAX */
#define GBX_ABEA_FREQ_KEY_BITS     4   /*        a key does not fit pos_bits / contig_bits */
#define GBX_ABEA_FREQ_ITEMS        8   /*        n_items is not what the count pass found */
#define GBX_ABEA_FREQ_CPGS   1         /* header kind: num_cpgs / num_cpgs_in_group */
#define GBX_ABEA_FREQ_MOTIFS 2         /*              num_motifs / num_motifs_in_group */
/* Records -> table on the device, on the caller's stream; nothing is synchronised.  pass COUNT writes d_item_off[n_records + 1]
 * (exclusive scan, the total in entry n_records and in d_counts[0]); the caller reads the total and passes it as n_items to
 * the later passes.  pass REDUCE makes the items, sorts them stably by key with as many 8-bit passes as pos_bits (1..31, for
 * start and end) and contig_bits (1..31) need, and writes d_counts[1..4]; pass FILL writes the sites and the arena, nothing
 * past site_cap sites and nothing of a sequence that would end past seq_cap.  d_work: gbx_abea_freq_work(n_records, n_items)
 * bytes, the same buffer in REDUCE and FILL (COUNT needs gbx_abea_freq_work(n_records, 0)).  d_counts: GBX_ABEA_FREQ_NCOUNTS
 * int64.  An n_items other than the count pass's total sets GBX_ABEA_FREQ_ITEMS: a record whose items would end past it
 * writes none, and the table means nothing then. */
int64_t gbx_abea_freq_work(int64_t n_records, int64_t n_items);
int gbx_abea_freq_device(int pass, int64_t n_records, const gbx_abea_freq_record *d_records, const char *d_rec_arena,
                         double threshold, int split_groups, int pos_bits, int contig_bits, int64_t n_items, void *d_work,
                         int64_t *d_item_off, int64_t *d_counts, int64_t site_cap, gbx_abea_freq_site *d_sites, int64_t seq_cap,
                         char *d_seq_arena, void *stream);
/* Pageable host buffers (one device).  Checked before the device is touched, GBX_ERR_ARG naming the lowest offender:
 * negative contig, start, end or n_cpg, a sequence outside the arena.  *n_sites and *seq_bytes: the table's sizes; one above
 * its capacity gives GBX_ERR_ARG with the needs there (call with 0 / NULL to size). */
int gbx_abea_freq_host(int64_t n_records, const gbx_abea_freq_record *records, const char *rec_arena, int64_t rec_arena_bytes,
                       double threshold, int split_groups, int64_t site_cap, gbx_abea_freq_site *sites, int64_t *n_sites,
                       int64_t seq_cap, char *seq_arena, int64_t *seq_bytes);
/* call-methylation's sites and scores -> records, without the text: site s of read r becomes the record (contig_of_read[r],
 * start_position, end_position, n_cpg, llr, context) unless (clip_start != -1 && start_position < clip_start) ||
 * (clip_end != -1 && end_position >= clip_end), the filter of gbx_abea_meth_tsv_host.  llr is what meth-freq reads from the
 * text: the double scores[2 s + 1] - scores[2 s] rounded to two decimals as "%.2lf" prints it (the exact binary value, ties to
 * even) and divided by 100.0; from 2^46 in magnitude, and for inf / NaN, the value itself.  The context is ctx_len bytes at
 * ctx_off of the read's reference segment, each mapped as the TSV writer maps it.  pass COUNT writes d_off[2 (n_sites + 1)]:
 * the record offsets, then the byte offsets (totals in the last entry of each); pass FILL writes the records and the arena,
 * nothing past rec_cap / seq_cap.  d_work: gbx_abea_freq_records_work(n_sites) bytes.  Nothing is synchronised. */
int64_t gbx_abea_freq_records_work(int64_t n_sites);
int gbx_abea_freq_records_device(int pass, int64_t n_sites, const gbx_abea_meth_site *d_sites, const float *d_scores,
                                 int64_t n_reads, const int32_t *d_contig_of_read, const int64_t *d_ref_off,
                                 const int32_t *d_ref_len, const char *d_ref_arena, int32_t clip_start, int32_t clip_end,
                                 void *d_work, int64_t *d_off, int64_t rec_cap, gbx_abea_freq_record *d_records, int64_t seq_cap,
                                 char *d_seq_arena, void *stream);
/* The arrays gbx_abea_call_methylation_host returns.  Checked first, GBX_ERR_ARG naming the lowest offender: a site's read, a
 * context outside the read's segment, a negative contig.  Capacities as gbx_abea_freq_host. */
int gbx_abea_freq_records_host(int64_t n_sites, const gbx_abea_meth_site *sites, const float *scores, int64_t n_reads,
                               const int32_t *contig_of_read, const int64_t *ref_off, const int32_t *ref_len,
                               const char *ref_arena, int32_t clip_start, int32_t clip_end, int64_t rec_cap,
                               gbx_abea_freq_record *records, int64_t *n_records, int64_t seq_cap, char *seq_arena,
                               int64_t *seq_bytes);
/* Two tables -> the table of the concatenated input, A's records first: both become items (weights called_sites and
 * called_sites_methylated, group_size and sequence as they stand), then the same sort and reduce, so a key in both keeps A's
 * group size and sequence.  (A table holds no site whose records all had weight 0, so such records of A no longer fix a
 * group size of 0 for B's calls: the one difference from the concatenated input, at threshold 0 only.)  pass REDUCE and / or FILL; d_work: gbx_abea_freq_work(n_a + n_b, n_a + n_b) bytes. */
int gbx_abea_freq_merge_device(int pass, int64_t n_a, const gbx_abea_freq_site *d_sites_a, const char *d_arena_a, int64_t n_b,
                               const gbx_abea_freq_site *d_sites_b, const char *d_arena_b, int pos_bits, int contig_bits,
                               void *d_work, int64_t *d_counts, int64_t site_cap, gbx_abea_freq_site *d_sites, int64_t seq_cap,
                               char *d_seq_arena, void *stream);
int gbx_abea_freq_merge_host(int64_t n_a, const gbx_abea_freq_site *sites_a, const char *arena_a, int64_t arena_a_bytes,
                             int64_t n_b, const gbx_abea_freq_site *sites_b, const char *arena_b, int64_t arena_b_bytes,
                             int64_t site_cap, gbx_abea_freq_site *sites, int64_t *n_sites, int64_t seq_cap, char *seq_arena,
                             int64_t *seq_bytes);
/* Table -> the text meth-freq prints (freq.c:381-416): with_header the header of `header_kind` first, then per site
 * "%s\t%d\t%d\t%d\t%d\t%d\t%.3lf\t%s\n" with the frequency (double)called_sites_methylated / called_sites rounded as printf
 * rounds it.  Contig c's name is d_names[d_name_off[c] .. d_name_off[c + 1]); a contig outside 0 .. n_contigs - 1 prints
 * an empty name.  pass COUNT (GBX_ABEA_FREQ_COUNT) writes d_line_off[n_sites + 2]: entry 0 the header's place (0), entry s + 1 site s's
 * line, the last entry the bytes of the whole text; pass FILL writes the lines that end inside cap.  d_work:
 * gbx_abea_freq_tsv_work(n_sites) bytes.  Nothing is synchronised. */
int64_t gbx_abea_freq_tsv_work(int64_t n_sites);
int gbx_abea_freq_tsv_device(int pass, int64_t n_sites, const gbx_abea_freq_site *d_sites, const char *d_seq_arena,
                             int64_t n_contigs, const int64_t *d_name_off, const char *d_names, int header_kind, int with_header,
                             void *d_work, int64_t *d_line_off, int64_t cap, char *d_out, void *stream);
/* Host buffers.  Checked first: contigs inside contig_names, sequences inside the arena, called_sites > 0.  *n_bytes: the
 * bytes of text; more than cap: GBX_ERR_ARG with the need there (call with 0 / NULL to size). */
int gbx_abea_freq_tsv_host(int64_t n_sites, const gbx_abea_freq_site *sites, const char *seq_arena, int64_t seq_bytes,
                           int64_t n_contigs, const char *const *contig_names, int header_kind, int with_header, int64_t cap,
                           char *out, int64_t *n_bytes);
/* Host only: the call-methylation TSV -> records, as get_tsv_line reads it (freq.c:175-251): one of the four headers (with /
 * without strand, num_cpgs / num_motifs -> *header_kind), fields cut as strtok cuts them, atoi and strtod of the C library.
 * The contig names come back sorted by strcmp, NUL-terminated one after the other in `names`; a record's contig is its
 * name's rank.  Where the reference exits (no header, a bad header, a missing column, an extra column, a negative coordinate
 * or count) the return is GBX_ERR_ARG, gbx_last_error() is the reference's message and *bad_line its line number (0 for the
 * header); a contig name holding ':' (the reference's own key breaks on it) is GBX_ERR_UNSUPPORTED.  counts[4]: records,
 * sequence bytes, contigs, name bytes; one above its capacity gives GBX_ERR_ARG with *bad_line = -1 and the needs in counts
 * (call with 0 / NULL to size). */
int gbx_abea_freq_parse_host(const char *text, int64_t n_bytes, int64_t rec_cap, gbx_abea_freq_record *records, int64_t seq_cap,
                             char *seq_arena, int64_t name_cap, char *names, int64_t *counts, int *header_kind,
                             int64_t *bad_line);

/* abea, calibration and the event-alignment record: what f5c runs per read between align() and the methylation score.
 * Replaces  int32_t postalign(alignment, base_to_event_map, events_per_base, sequence, n_kmers, event_alignment, n_events)
 *                                                                                              align.c:550-650
 *           bool recalibrate_model(pore_model, et, scallings, alignment_output, num_alignments, scale_var = 1)
 *                                                                                              align.c:655-762
 *           with the three QC rules of scaling_single                                          f5c.c:1262-1330
 *           int32_t get_event_alignment_record(record, read_length, base_to_event_map, &aligned_events)   meth.c:15-185
 * Bit for bit the reference's order of operations: the five sums of the normal equations and the residual sum are double
 * accumulations in k-mer order, division and square root are the correctly rounded double ones.  The event_alignment_t
 * array is not materialised: a k-mer with events gives stop - start + 1 records, the first of them 'M' (its event:
 * start) when its rank differs from the rank of the previous k-mer with events, every other one 'E' and in no sum.
 * The one assumption: the pairs of a read never decrease in either field, as align() writes them (align.c:476-487); the
 * host entry checks it.
 * Per read r: flags[r] = GBX_ABEA_FAILED_ALIGNMENT when n_pairs[r] == 0 (map all -1, events_per_base 0, scalings
 * untouched); GBX_ABEA_FAILED_CALIBRATION with fewer than 200 M states (scale, shift unchanged; var, which the reference
 * leaves uninitialised there, is 0) or when the recalibrated var is above 2.5 (scale, shift and var are overwritten
 * all the same); GBX_ABEA_FAILED_QUALITY_CHK when events_per_base > 5.0, tested only when calibration did not fail.
 * The map: int32 (start, stop) per k-mer, (-1, -1) for a k-mer without events; read r's seq_len[r] - 5 entries at
 * map + 2 * seq_off[r] (ints), the slots behind them unspecified.  events_per_base = (double)(max_event - min_event) /
 * n_kmers with min_event starting at INT32_MAX and max_event at 0, as written. */
#define GBX_ABEA_FAILED_CALIBRATION 1   /* FAILED_CALIBRATION, f5c.h:49 */
#define GBX_ABEA_FAILED_ALIGNMENT   2   /* FAILED_ALIGNMENT,   f5c.h:50 */
#define GBX_ABEA_FAILED_QUALITY_CHK 4   /* FAILED_QUALITY_CHK, f5c.h:51 */
#define GBX_ABEA_RECORD_COUNT 1         /* pass: the record lengths and rec_off */
#define GBX_ABEA_RECORD_FILL  2         /* pass: the records at the rec_off of a count pass */

/* Device entry, on what gbx_abea_align_device leaves: d_event_off ABSOLUTE as there, read r's pairs at d_pairs +
 * 2 * d_event_off[r], d_n_pairs[r] of them.  d_scale / d_shift are never read; for a recalibrated read they are overwritten,
 * for every other read they are left as they were.
 * d_var64 is the double that var was stored from (its logarithm is taken on the host, below).  d_map holds 2 ints per
 * base of the arena.  Nothing is synchronised. */
int gbx_abea_calib_device(int64_t n_reads, const int64_t *d_seq_off, const int32_t *d_seq_len, const char *d_seq_arena,
                          const int64_t *d_event_off, const float *d_event_mean, const gbx_abea_model *d_models,
                          const gbx_abea_pair *d_pairs, const int32_t *d_n_pairs, float *d_scale, float *d_shift,
                          float *d_var, double *d_var64, int32_t *d_map, double *d_events_per_base,
                          int32_t *d_n_event_alignment, int32_t *d_n_m_state, int32_t *d_flags, void *stream);
/* log_var[r] = (float)log(var64[r]) (scallings->log_var, align.c:749: a double logarithm, taken with the host C library
 * so that it carries the reference's bits) for the reads recalibration ran on (n_m_state[r] >= 200), 0 for the others. */
int gbx_abea_calib_logvar_host(int64_t n_reads, const double *var64, const int32_t *n_m_state, float *log_var);
/* Host-buffer entry (one device).  events: the 24-byte records; pairs as gbx_abea_align_host returns them (2 *
 * event_off[n_reads] slots); map: 2 * seq_bytes ints.  Checked before the device is touched, GBX_ERR_ARG naming the
 * lowest offender: reads inside the arena with at least KMER bases, 0 <= n_pairs <= 2 * n_events, every pair inside
 * the read's k-mers and events, and no pair below the one before it in either field. */
int gbx_abea_calib_host(int64_t n_reads, const int64_t *seq_off, const int32_t *seq_len, const char *seq_arena,
                        int64_t seq_bytes, const int64_t *event_off, const gbx_abea_event *events,
                        const gbx_abea_model *models, const gbx_abea_pair *pairs, const int32_t *n_pairs, float *scale,
                        float *shift, float *var, float *log_var, double *var64, int32_t *map, double *events_per_base,
                        int32_t *n_event_alignment, int32_t *n_m_state, int32_t *flags);

/* The event-alignment record of read r from its BAM-encoded CIGAR (len << 4 | op; cigar[cigar_off[r] .. cigar_off[r+1])),
 * pos[r], rc[r], seq_len[r] and its map: get_aligned_segments (M, = and X advance both positions and emit a pair, D the
 * reference, I and S the read, H nothing), the boundary skip (read_pos < 6 or read_pos + 6 >= read_length), the strand
 * flip (read_length - read_pos - 6), get_closest_event_to (backwards over k_idx .. max(0, k_idx - 1000) + 1, else forwards
 * over k_idx .. min(k_idx + 1000, n_kmers - 1) - 1; -1 is a legal result) and the degenerate rule (first event == last
 * event: length 0).  Output: the compact record gbx_abea_meth_sites_host consumes, rec_off[n_reads + 1] and (ref_pos,
 * event index) pairs.
 * Device entry.  pass = COUNT writes d_rec_off[n_reads + 1] and the workspace d_near (2 ints per base of the arena, like
 * the map); pass = FILL writes the records of a count pass over the same input; a read whose record would end past
 * rec_cap is left unwritten.  COUNT | FILL does both (a record never has more than seq_len - 12 pairs).  d_flags may be
 * NULL; a read with a non-zero flag gets an empty record (meth_single, f5c.c:1376).  An operation the reference refuses
 * (N, P, a code above 8) advances nothing here.  Nothing is synchronised. */
int gbx_abea_event_record_device(int pass, int64_t n_reads, const int64_t *d_cigar_off, const uint32_t *d_cigar,
                                 const int32_t *d_pos, const uint8_t *d_rc, const int64_t *d_seq_off, const int32_t *d_seq_len,
                                 const int32_t *d_map, const int32_t *d_flags, int32_t *d_near, int64_t *d_rec_off,
                                 gbx_abea_pair *d_rec, int64_t rec_cap, void *stream);
/* Host-buffer entry (one device).  map: 2 * seq_bytes ints; flags may be NULL.  *n_rec = the pairs of all records; more
 * than rec_cap gives GBX_ERR_ARG with the needed count there and in gbx_last_error() (rec_off is valid then; call with
 * 0 / NULL to size).  Refused with GBX_ERR_ARG where the reference exits or asserts: operation N (meth.c:54-58), P or a
 * code above 8 (meth.c:65-68), more aligned bases than seq_len (meth.c:135). */
int gbx_abea_event_record_host(int64_t n_reads, const int64_t *cigar_off, const uint32_t *cigar, const int32_t *pos,
                               const uint8_t *rc, const int64_t *seq_off, const int32_t *seq_len, int64_t seq_bytes,
                               const int32_t *map, const int32_t *flags, int64_t *rec_off, int64_t rec_cap,
                               gbx_abea_pair *rec, int64_t *n_rec);

/* call-methylation from raw signal in one call (one device): events -> scalings -> align -> calibration -> record ->
 * site planner -> score, what f5c runs per batch between reading its input and writing its TSV (process_db,
 * f5c.c:1219-1400, mode 0).  Signal, reads and model as gbx_abea_signal_align_host; the CpG model as
 * gbx_abea_meth_score_host; CIGARs, pos and rc as gbx_abea_event_record_host; the reference segments as
 * gbx_abea_meth_sites_host with ref_start_pos = pos.  The events, their means and the scalings stay on the device: what
 * comes down is the event counts, the per-read calibration (log_var is taken on the host) and the record of the
 * unflagged reads; the site planner runs on the host and its jobs go back up.
 * Per read: flags (a read without events: GBX_ABEA_FAILED_ALIGNMENT), scale, shift, var, events_per_base, status (the
 * event stage's).  Sites of all unflagged reads in read order, scores[2 s] the unmethylated and scores[2 s + 1] the
 * methylated score of site s; ctx_off refers to the read's reference segment.  More sites than site_cap: GBX_ERR_ARG
 * with the needed count in *n_sites (the per-read outputs are valid then; call with 0 / NULL to size). */
int gbx_abea_call_methylation_host(int64_t n_reads, const int16_t *raw, const int64_t *raw_off, const float *range,
                                   const float *digitisation, const float *offset, const int64_t *seq_off,
                                   const int32_t *seq_len, const char *seq_arena, int64_t seq_bytes,
                                   const gbx_abea_model *models, const gbx_abea_model *cpg_model, const int64_t *cigar_off,
                                   const uint32_t *cigar, const int32_t *pos, const uint8_t *rc, const int64_t *ref_off,
                                   const int32_t *ref_len, const char *ref_arena, int32_t *flags, int32_t *status,
                                   float *scale, float *shift, float *var, double *events_per_base, int64_t site_cap,
                                   gbx_abea_meth_site *sites, float *scores, int64_t *n_sites);

/* abea, eventalign: what f5c eventalign runs per read behind the calibration in place of the methylation score
 * (meth_single, f5c.c:1381-1387, mode 1).
 * Replaces  std::vector<event_alignment_t> align_read_to_ref(params, ref)        eventalign.c:1263-1540 (realign_read)
 *           profile_hmm_align, the Viterbi fill and its traceback                 eventalign.c:345-911
 *           EventalignSummary summarize_alignment(...)                            eventalign.c:1580-1642
 *           void emit_event_alignment_tsv(...) and its header                     eventalign.c:1651-1662, 1853-1938
 * A read is realigned in segments of about 100 reference bases: the aligned pairs of its CIGAR (M, = and X; no 6-base
 * boundary skip; trimmed to [region_start, region_end] when neither is -1, then to read_pos <= seq_len - 6) give the
 * segment's reference bases and, through get_closest_event_to, its events; a three-state profile HMM (M, B, K per k-mer) is
 * filled with float max in place of the log-sum, on the NUCLEOTIDE model (4096 k-mers, N and every other byte rank as A);
 * `from` of a cell is the LAST of its six candidates that equals their maximum (six -inf: HMT_FROM_SOFT); the traceback
 * starts at M of the last k-mer in the last row; the first 50 states that are not K and not on the segment's first event are
 * emitted (all of them when the segment reaches the last pair) and the next segment starts at the last one emitted.
 * Bit for bit the reference's paths: the emission is the float one of eventalign.c:293-338 with its division, the transition
 * logarithms and log(1 - TRANS_START_TO_CLIP) are taken with the host C library.
 * A record: ref_pos = curr_start_ref + kmer_idx, event_idx (the read's own index), state 'M' or 'B'.  ref_kmer is the six
 * disambiguated upper-case bases at ref_pos; model_kmer is NNNNNN for B, else ref_kmer, reverse-complemented on an rc read.
 * A read has at most n_events records, read r's at rec + event_off[r] (ABSOLUTE on the device entry), n_rec[r] of them.
 * Status bits of a read; with any of them the read keeps the records of the segments before:
 *   ROWS       a segment has more events than the workspace holds rows for (rows_cap; the host entries use
 *              GBX_ABEA_EVENTALIGN_ROWS and the caller of the device entry sizes the workspace)
 *   UNDEFINED  the reference would assert or read out of range: the traceback's start cell is -inf (or not a number),
 *              get_closest_event_to gives -1 for the first or the last event, an event index outside the read, a segment
 *              outside the reference segment, events that run against rc (eventalign.c:363), a path that leaves the matrix
 *   BOUND      a loop hit its bound (segments <= n_events + 1, traceback steps <= rows + k-mers + 1)
 * One deviation: a segment of length <= 0 (curr_start_ref inside a deletion of more than 100 bases; the reference calls
 * substr with a negative length) ends the read like a segment of fewer than 12 bases. */
#define GBX_ABEA_EVENTALIGN_ROWS       1024   /* rows_cap of the host entries */
#define GBX_ABEA_EVENTALIGN_SLABS      3072   /* wavefronts (and backtrack slabs) of a launch, at most */
#define GBX_ABEA_EVENTALIGN_MAX_KMERS  96     /* align_stride 100 + 1 bases */
#define GBX_ABEA_EVENTALIGN_ST_ROWS      1
#define GBX_ABEA_EVENTALIGN_ST_UNDEFINED 2
#define GBX_ABEA_EVENTALIGN_ST_BOUND     4
typedef struct gbx_abea_eventalign_rec { int32_t ref_pos, event_idx, state; } gbx_abea_eventalign_rec;
typedef struct gbx_abea_eventalign_summary {   /* EventalignSummary, f5c.h:222-245, without the NM tag (the caller's) */
    int32_t num_events, num_steps, num_stays, num_skips;
    double sum_duration, sum_z_score;
    int32_t reference_span, pad_;
} gbx_abea_eventalign_summary;

/* trans[r][GBX_ABEA_METH_NTRANS] as gbx_abea_meth_plan_host lays them out (calculate_transitions, eventalign.c:171-240: the
 * same float arithmetic and float logarithms), from events_per_base; host C library. */
int gbx_abea_eventalign_trans_host(int64_t n_reads, const double *events_per_base, float *trans);
/* 256 bytes of header, 16 bytes per CIGAR operation and min(n_reads, GBX_ABEA_EVENTALIGN_SLABS) slabs of rows_cap x 192 bytes */
size_t gbx_abea_eventalign_workspace_bytes(int64_t n_reads, int64_t n_cigar_total, int64_t rows_cap);
/* Device entry, on what gbx_abea_calib_device (map, scalings, var, flags), gbx_abea_calib_logvar_host (log_var) and the count
 * pass of gbx_abea_event_record_device (near) leave.  d_event_off ABSOLUTE; d_cigar_off[0] = 0 .. d_cigar_off[n_reads] =
 * n_cigar_total; d_ref_off / d_ref_len: the reference segment of read r starts at pos[r].  d_order: the reads in the order
 * they are to be drawn (longest first), or NULL for 0, 1, ...  Reads with a non-zero flag, without events or without pairs
 * get n_rec 0, status 0.  An operation the reference refuses (N, P, a code above 8) advances nothing.  Nothing is synchronised. */
int gbx_abea_eventalign_device(int64_t n_reads, const int64_t *d_seq_off, const int32_t *d_seq_len, const int64_t *d_event_off,
                               const float *d_event_mean, const gbx_abea_model *d_models, const float *d_scale, const float *d_shift,
                               const float *d_var, const float *d_log_var, const float *d_trans, const int32_t *d_map,
                               const int32_t *d_near, const int32_t *d_flags, const int64_t *d_cigar_off, const uint32_t *d_cigar,
                               const int32_t *d_pos, const uint8_t *d_rc, const int64_t *d_ref_off, const int32_t *d_ref_len,
                               const char *d_ref_arena, int32_t region_start, int32_t region_end, const int32_t *d_order,
                               gbx_abea_eventalign_rec *d_rec, int32_t *d_n_rec, int32_t *d_status, int64_t *d_counts /* [3] or NULL: segments, cells, traceback steps */,
                               int64_t n_cigar_total, int64_t rows_cap, void *d_work, size_t work_bytes, void *stream);
/* Host-buffer entry (one device), on what gbx_abea_calib_host returned: events (24-byte records), scale, shift, var, log_var,
 * events_per_base, map (2 * seq_bytes ints), flags.  rec holds event_off[n_reads] - event_off[0] records, read r's at rec +
 * event_off[r] - event_off[0].  Checked before the device is touched, GBX_ERR_ARG naming the lowest offender: reads inside
 * the arena, CIGARs as gbx_abea_event_record_host checks them (operation N is refused), reference bases outside the IUPAC
 * alphabet (the reference asserts), region_start > region_end. */
int gbx_abea_eventalign_host(int64_t n_reads, const int64_t *seq_off, const int32_t *seq_len, int64_t seq_bytes,
                             const int64_t *event_off, const gbx_abea_event *events, const gbx_abea_model *models, const float *scale,
                             const float *shift, const float *var, const float *log_var, const double *events_per_base,
                             const int32_t *map, const int32_t *flags, const int64_t *cigar_off, const uint32_t *cigar,
                             const int32_t *pos, const uint8_t *rc, const int64_t *ref_off, const int32_t *ref_len,
                             const char *ref_arena, int32_t region_start, int32_t region_end, gbx_abea_eventalign_rec *rec,
                             int32_t *n_rec, int32_t *status);
/* summarize_alignment per read (host only, no device): event lengths in samples, z-scores of the M records. */
int gbx_abea_eventalign_summary_host(int64_t n_reads, const int64_t *event_off, const gbx_abea_event *events,
                                     const gbx_abea_model *models, const float *scale, const float *shift, const float *var,
                                     const uint8_t *rc, const int32_t *pos, const int64_t *ref_off, const int32_t *ref_len,
                                     const char *ref_arena, const gbx_abea_eventalign_rec *rec, const int32_t *n_rec,
                                     gbx_abea_eventalign_summary *out);
/* The TSV of one read (host only): emit_event_alignment_tsv's lines, behind the header line when `header` is set.  Formatted
 * with the C library.  Returns through *need the bytes of the text (without a terminator); more than cap: GBX_ERR_ARG, call
 * again with room.  write_samples != 0 is refused (the reference asserts). */
int gbx_abea_eventalign_tsv_host(const gbx_abea_event *events, int64_t n_events, const gbx_abea_model *models, float scale, float shift,
                                 float var, int rc, int32_t pos, const char *ref, int32_t ref_len,
                                 const gbx_abea_eventalign_rec *rec, int32_t n_rec, int header, int print_read_names, int scale_events,
                                 int write_samples, int64_t read_index, const char *read_name, const char *ref_name, float sample_rate,
                                 char *text, int64_t cap, int64_t *need);
/* eventalign from raw signal in one call (one device): events -> scalings -> align -> calibration -> near table -> eventalign.
 * Inputs as gbx_abea_call_methylation_host without the CpG model.  The events, their means, the map and the scalings stay on
 * the device; the per-read calibration comes down (log_var and the transitions are taken on the host) and, at the end, the
 * event records (events: event_cap of them; read r's at events + event_off[r]) and the eventalign records beside them (rec:
 * event_cap).  More events than event_cap: GBX_ERR_ARG with the count in *n_events_total, as gbx_abea_events_host. */
int gbx_abea_eventalign_from_signal_host(int64_t n_reads, const int16_t *raw, const int64_t *raw_off, const float *range,
                                         const float *digitisation, const float *offset, const int64_t *seq_off,
                                         const int32_t *seq_len, const char *seq_arena, int64_t seq_bytes,
                                         const gbx_abea_model *models, const int64_t *cigar_off, const uint32_t *cigar,
                                         const int32_t *pos, const uint8_t *rc, const int64_t *ref_off, const int32_t *ref_len,
                                         const char *ref_arena, int32_t region_start, int32_t region_end, int32_t *flags,
                                         int32_t *status, float *scale, float *shift, float *var, float *log_var,
                                         double *events_per_base, int64_t *event_off, gbx_abea_event *events, int64_t event_cap,
                                         int64_t *n_events_total, gbx_abea_eventalign_rec *rec, int32_t *n_rec, int32_t *ea_status);

/* --------------------------------------------------------------------- fmi
 * SMEM seeding on the FM-index of reference + reverse complement (second half): the three
 * seeding rounds bwa-mem2 runs per batch of reads and the driver times,
 *   R/benchmarks/fmi/fmi.cpp:218-228  FMI_search::getSMEMsAllPosOneThread   SMEMs from every start position
 *   R/benchmarks/fmi/fmi.cpp:230-254  re-seeding: getSMEMsOnePosOneThread from the middle of every SMEM of at least
 *                                     split_len bases with at most split_width hits, min_intv = hits + 1
 *   R/benchmarks/fmi/fmi.cpp:255-266  FMI_search::bwtSeedStrategyAllPosOneThread (max_intv, minSeedLen + 1)
 *   R/benchmarks/fmi/fmi.cpp:270-278  rid += batch offset, FMI_search::sortSMEMs
 * FMI_search lives in tools/bwa-mem2 (an empty submodule here): the arithmetic follows bwa-mem2's published
 * src/FMI_search.cpp (backwardExt over the CP_OCC checkpoints of 64 BWT symbols) - parity UNPINNED by a compiled
 * reference, see oracle/fmi_oracle.c.
 * The three rounds and the sort only ever combine SMEMs of one read, and batches are contiguous rid ranges sorted by
 * rid first, so the job's result is independent of the batch size: for every read, in rid order, its SMEMs of all
 * three rounds sorted by (m ascending, n descending).  Records equal in (rid, m, n) are equal in every field.
 */
typedef struct gbx_fmi_cp_occ {      /* bwa-mem2 CP_OCC (FMI_search.h): one checkpoint per 64 BWT symbols, 64 bytes */
    int64_t  cp_count[4];            /* occurrences of A, C, G, T in bwt[0, 64 i) */
    uint64_t one_hot_bwt_str[4];     /* bit 63 - j set iff bwt[64 i + j] is that base */
} gbx_fmi_cp_occ;
typedef struct gbx_fmi_index {       /* the fields of FMI_search the search reads (load_index) */
    int64_t ref_seq_len;             /* reference_seq_len: 2 x genome length + 1 (the sentinel) */
    int64_t count[5];                /* first SA row of every base, sentinel row included: count[0] = 1, count[4] = ref_seq_len */
    int64_t sentinel_index;          /* SA row whose BWT symbol is the sentinel */
    const gbx_fmi_cp_occ *cp_occ;    /* (ref_seq_len >> 6) + 1 checkpoints; host pointer for *_host, device pointer for *_device */
} gbx_fmi_index;
typedef struct gbx_fmi_smem {        /* bwa-mem2 SMEM (FMI_search.h), 40 bytes */
    uint32_t rid;                    /* read */
    uint32_t m, n;                   /* query interval [m, n], both inclusive (the driver prints [m, n + 1)) */
    uint32_t pad_;
    int64_t  k, l, s;                /* SA interval of the match, of its reverse complement, and their size */
} gbx_fmi_smem;
typedef struct gbx_fmi_params {      /* fmi.cpp:135-140,178 */
    int32_t min_seed_len;            /* argv[4]; the benchmark scripts pass 19 */
    int32_t split_width;             /* 10 */
    int32_t split_len;               /* (int)(min_seed_len * 1.5 + .499) */
    int32_t max_mem_intv;            /* 20 */
} gbx_fmi_params;
void gbx_fmi_default_params(gbx_fmi_params *p, int32_t min_seed_len);

/* Host-buffer entry: reads as base codes 0..3 (4 = ambiguous, fmi.cpp:113-124; the CONTRACT is codes 0..4 - larger values are not
 * checked and their treatment is unspecified), read r = enc[read_off[r] ..+ read_len[r]).
 * out receives the SMEMs (out_cap records; GBX_ERR_ARG with the needed count in gbx_last_error() when it is too small),
 * smem_off[n_reads + 1] (nullable) where each read's run starts, *n_out the total. */
int gbx_fmi_smem_host(const gbx_fmi_index *idx, const gbx_fmi_params *p, int64_t n_reads, const uint8_t *enc, int64_t enc_bytes,
                      const int64_t *read_off, const int32_t *read_len, gbx_fmi_smem *out, int64_t out_cap,
                      int64_t *smem_off, int64_t *n_out);

/* Device path.  The checkpoints are re-laid for the device once per index (gbx_fmi_index_bytes / gbx_fmi_index_build:
 * the count and the one-hot word of a base side by side, so that the four lanes of a read fetch a checkpoint as one
 * 64-byte line).  d_smem_off[n_reads + 1] and d_n_out (one int64) are written on the device; *d_n_out greater than
 * out_cap means the output did not fit (nothing beyond out_cap is written). */
size_t gbx_fmi_index_bytes(int64_t ref_seq_len);
int gbx_fmi_index_build(const gbx_fmi_index *idx_with_device_cp_occ, void *d_index, size_t index_bytes, void *stream);
size_t gbx_fmi_workspace_bytes(int64_t n_reads, int32_t max_read_len, int32_t min_seed_len);
int gbx_fmi_smem_device(const gbx_fmi_index *idx, const void *d_index, const gbx_fmi_params *p, int64_t n_reads,
                        int32_t max_read_len, const uint8_t *d_enc, const int64_t *d_read_off, const int32_t *d_read_len,
                        gbx_fmi_smem *d_out, int64_t out_cap, int64_t *d_smem_off, int64_t *d_n_out,
                        void *d_work, size_t work_bytes, void *stream);
/* A read's SMEMs wait in a slot of max(48, 4 * max_read_len / min_seed_len + 16) records for the pack pass.  *worst = 0, or
 * a lower bound of the largest count a read of the last gbx_fmi_smem_device call on this workspace asked for when that was
 * more (its surplus records, and what the re-seeding round would have made of them, are missing from the output then:
 * very repetitive text, long reads with short seeds).  The host entry runs such a job again with larger slots until
 * every read fits.  GBX_ERR_ARG when a read was longer than the max_read_len the call was given (such a read gets no SMEMs). */
int gbx_fmi_overflow(const void *d_work, int64_t *worst, void *stream);
/* backwardExt calls (checkpoint look-ups: two 64-byte lines each) of the last gbx_fmi_smem_device call on this workspace. */
int gbx_fmi_extensions(const void *d_work, int64_t *ext, void *stream);
/* gbx_fmi_smem_host keeps the device copy of an index between calls (a caller hands over the same tables for every batch
 * of reads, fmi.cpp:218), found again by content - the index scalars and a fingerprint of 256 checkpoints - not by address;
 * at most four idle copies per device; this frees the ones no call is using (and the suffix-array samples gbx_fmi_sal_host
 * keeps alike). */
int gbx_fmi_host_release(void);

/* ---- suffix-array lookup of SMEM hits (bwa-mem2's FMI_search::get_sa_entry, the step between seeding and extension)
 * text = genome + reverse complement, n = 2 L, ref_seq_len = n + 1; SA row 0 is the sentinel suffix (SA[0] = n) and the
 * BWT symbol at sentinel_index is the sentinel.  Samples as a .bwt.2bit.64 file stores them: the 40-bit value
 * ms_byte[i] << 32 | ls_word[i] is SA[i << sa_compx]; sa_compx 3 (n_sa = (ref_seq_len >> 3) + 1) or 0 (n_sa = ref_seq_len).
 * SA[r] of any row: while r is not sampled, step r <- LF(r) = count[b] + occ_b(r) (b the BWT symbol at r) and add 1 to an
 * offset t; a walk that reaches the sentinel row gives t, one that reaches a sampled row r' gives sample(r') + t.
 * Hits of an SMEM [k, k + s) follow bwa-mem's mem_chain sampling with max_occ (bwa's default 500): step = s > max_occ ?
 * s / max_occ : 1, rows k + i step for i = 0, 1, ... while i step < s and i < max_occ - min(s, max_occ) hits; max_occ <= 0:
 * every row.  SMEM j's hits go to pos[pos_off[j] .. pos_off[j + 1]) in increasing row order (pos_off: n_smem + 1 entries),
 * as raw text coordinates in [0, n] (the strand split, bwa's bns_depos, is the caller's); the output does not depend on
 * the scheduling.  An SMEM is bad unless k >= 0, s >= 1 and k + s <= ref_seq_len. */
typedef struct gbx_fmi_sa {
    int32_t sa_compx;                /* 3 or 0 */
    int64_t n_sa;                    /* (ref_seq_len >> 3) + 1, or ref_seq_len */
    const int8_t *ms_byte;           /* n_sa upper bytes; host pointers for *_host, device pointers for gbx_fmi_sa_build */
    const uint32_t *ls_word;         /* n_sa lower words */
} gbx_fmi_sa;

/* Host-buffer entry.  Every SMEM is checked before the device is touched: a bad one gives GBX_ERR_ARG naming the lowest.
 * *n_pos = the hit count; more than pos_cap gives GBX_ERR_ARG with the needed count in gbx_last_error().  pos_off
 * (n_smem + 1, nullable).  The device copies of the index and of the samples are kept between calls, found by content
 * (gbx_fmi_host_release frees them).  Safe under concurrent host threads. */
int gbx_fmi_sal_host(const gbx_fmi_index *idx, const gbx_fmi_sa *sa, const gbx_fmi_smem *smems, int64_t n_smem, int32_t max_occ,
                     int64_t *pos, int64_t pos_cap, int64_t *pos_off, int64_t *n_pos);

/* Device path.  The samples are re-laid for the device once per index (gbx_fmi_sa_bytes / gbx_fmi_sa_build: 32 bits per
 * sample when ref_seq_len < 2^32, 64 otherwise - or always with GBX_FMI_WIDE=1, which also selects the 64-bit kernel; the
 * variable must be the same for the build and the lookups).  The SMEM count is read on the device (*d_n_smem, e.g. the
 * d_n_out of gbx_fmi_smem_device on the same stream; at most smem_cap SMEMs are looked up), so the two calls chain without a
 * host round trip.  d_pos_off holds smem_cap + 1 entries (those past the SMEM count repeat the total); *d_n_pos = the hit
 * count, greater than pos_cap when the output did not fit (nothing past pos_cap is written).  A bad SMEM is not walked:
 * its hits (as many as for min(s, ref_seq_len)) are -1. */
size_t gbx_fmi_sa_bytes(int64_t n_sa, int64_t ref_seq_len);
int gbx_fmi_sa_build(const gbx_fmi_sa *sa_with_device_arrays, int64_t ref_seq_len, void *d_sa, size_t sa_bytes, void *stream);
size_t gbx_fmi_sal_workspace_bytes(int64_t smem_cap, int64_t pos_cap);
int gbx_fmi_sal_device(const gbx_fmi_index *idx, const void *d_index, const gbx_fmi_sa *sa, const void *d_sa,
                       const gbx_fmi_smem *d_smems, const int64_t *d_n_smem, int64_t smem_cap, int32_t max_occ,
                       int64_t *d_pos, int64_t pos_cap, int64_t *d_pos_off, int64_t *d_n_pos, void *d_work, size_t work_bytes,
                       void *stream);
/* LF steps of the last gbx_fmi_sal_device call on this workspace: their total and the longest walk of one hit. */
int gbx_fmi_sal_steps(const void *d_work, int64_t *steps, int64_t *max_steps, void *stream);

/* ---- building the index on the device (the job of `bwa-mem2 index`).  genome: l_pac base codes 0..3 of one strand.
 * The text is the strand and its reverse complement, n = 2 l_pac symbols; its n + 1 suffixes include the empty one, which sorts
 * first.  Suffix array by prefix doubling on radix sorts, then the BWT, the checkpoints and the samples: count[], sentinel_index,
 * the (ref_seq_len >> 6) + 1 CP_OCC records (rows past the end match no base) and SA[i << sa_compx] split into ms_byte / ls_word
 * (rows past the end: 0), n_sa as in gbx_fmi_sa.  Positions and ranks are 32-bit: 2 l_pac + 1 <= 2^32 - 1, i.e. l_pac <=
 * 2147483647; above it every entry returns GBX_ERR_UNSUPPORTED (gbx_fmi_build_workspace_bytes: 0).  Checked on the host before
 * any device work, GBX_ERR_ARG naming the lowest offender: null pointers, l_pac < 1, sa_compx other than 3 or 0, a base code
 * above 3 (host entries; the device entry's contract), a workspace below gbx_fmi_build_workspace_bytes(l_pac).
 * The workspace is about 38.7 bytes per text symbol (DESIGN 3.17 has the formula).
 * info: int64[8] = count[0..4], sentinel_index, doubling rounds run, slots the first round had to sort.
 * The device entry reads one count per doubling round, so it synchronises the stream; it returns with all work queued. */
size_t gbx_fmi_build_workspace_bytes(int64_t l_pac);
int gbx_fmi_build_device(const uint8_t *d_genome, int64_t l_pac, int32_t sa_compx, void *d_cp_occ, int8_t *d_ms, uint32_t *d_ls,
                         uint8_t *d_text /* 2 l_pac bytes out, may be null */, int64_t *d_info, void *d_work, size_t work_bytes, void *stream);
/* The slots each doubling round of the calling thread's last build (any entry) sorted: *n_rounds of them, the first cap into
 * slots.  For measurements (scripts/time_mem_index.py). */
int gbx_fmi_build_rounds(int64_t *slots, int32_t cap, int32_t *n_rounds);
/* Host buffers in and out; fills idx->ref_seq_len, count, sentinel_index, idx->cp_occ = cp_occ and the caller's cp_occ / ms / ls
 * arrays.  info: the eight words, may be null.  Safe under concurrent host threads. */
int gbx_fmi_build_host(const uint8_t *genome, int64_t l_pac, int32_t sa_compx, gbx_fmi_index *idx, gbx_fmi_cp_occ *cp_occ,
                       int8_t *ms, uint32_t *ls, int64_t *info);

/* ---- seed chaining (bwa-mem's mem_chain, mem_chain_flt and the window of mem_chain2aln: the step between the suffix-array
 * lookup and gbx_bsw_extend_seeds_*).  UNPINNED by a compiled reference (bwa's source is not part of the reference tree):
 * the rules are restated in full in DESIGN 3.10 and tests/mem_chain_ref.py, and pinned by that restatement.
 * Per read r: its SMEMs smems[smem_off[r] .. smem_off[r+1]) in order, SMEM j's hits pos[pos_off[j] .. pos_off[j+1]) in order
 * (a hit of -1 is skipped), text coordinates in [0, 2 L), L = l_pac, forward strand [0, L).  A seed is (qbeg = m,
 * len = n + 1 - m, rbeg = hit).  Contigs: contig_off[n_contigs + 1], forward coordinates, strictly increasing from 0 to L.
 *   chaining  a seed whose interval crosses L or a contig boundary is skipped; `lower` = the chain with the greatest
 *             pos <= rbeg (pos = its first seed's rbeg; among equal pos the one created last: bwa's pick depends on its
 *             B-tree's shape); the seed merges into it (contained: dropped; same contig and strand, y >= 0, |x - y| <= w,
 *             x - last.len and y - last.len below max_chain_gap: appended) or starts a new chain
 *   l_rep     bwa's frac_rep numerator: the query bases covered by SMEMs with s > max_occ
 *   filter    weight = min(query cover, reference cover); chains below min_chain_weight go; the rest, by weight descending
 *             (ties: by pos, then creation), through mem_chain_flt's overlap scan with mask_level, drop_ratio (fp32) and
 *             min_seed_len, the rescue through `first`, and the max_chain_extend cap; kept = 3 no overlap, 2 overlaps a
 *             better chain, 1 the first chain shadowed by a kept one.  Alt contigs are not modelled (is_alt = 0).
 *   window    [rmax0, rmax1): min / max over the chain's seeds of the seed's start / end moved out by the rest of the read and
 *             the longest gap its score pays for (at most 2 w), clamped to [0, 2 L], cut at L and clipped to the contig
 * Output: the kept chains of every read, in read order and the filter's order, and for every seed of every kept chain, in
 * chain order then seed order, a gbx_bsw_seed (qoff = read_off[r], lq = read_len[r], roff = rmax0, rlen = rmax1 - rmax0,
 * rbeg relative to rmax0) for an extension whose ref arena is the 2 L-byte text and whose qer arena is the reads.
 * bwa's ordering of a chain's seeds by score, the skip of seeds an earlier alignment covers and seedcov are not done here:
 * they belong to gbx_mem_regs_* (below), which runs behind the extension. */
typedef struct gbx_mem_chain_params {
    int32_t w;                       /* 100 */
    int32_t max_chain_gap;           /* 10000 */
    int32_t max_occ;                 /* 500: the value the hits were sampled with (l_rep only) */
    int32_t min_seed_len;            /* 19 */
    int32_t min_chain_weight;        /* 0 */
    int32_t max_chain_extend;        /* 1 << 30 */
    float   mask_level, drop_ratio;  /* 0.5, 0.5 */
    int32_t a, o_del, e_del, o_ins, e_ins;   /* 1, 6, 1, 6, 1: the match score and gap costs of the extension */
    int32_t pad_;
} gbx_mem_chain_params;
void gbx_mem_chain_default_params(gbx_mem_chain_params *p);

typedef struct gbx_mem_chain {       /* 56 bytes */
    int64_t pos;                     /* the first seed's rbeg */
    int64_t seed_off;                /* its seeds are seeds[seed_off .. seed_off + n_seeds) */
    int64_t rmax0, rmax1;            /* the window, text coordinates */
    int32_t read, contig, n_seeds, weight, kept, pad_;
} gbx_mem_chain;

/* Device path.  All pointers are device pointers; asynchronous on `stream`, no host synchronisation inside.  The SMEM and
 * hit counts are read on the device (*d_n_smem, *d_n_pos: the d_n_out of gbx_fmi_smem_device and the d_n_pos of
 * gbx_fmi_sal_device on the same stream; at most smem_cap / pos_cap are used), so the call chains behind the two.
 * Written: d_chains[chain_cap], d_chain_off[n_reads + 1], d_seeds[seed_cap], d_l_rep[n_reads], *d_n_chains, *d_n_seeds.  A
 * count above its capacity reports the need: nothing past the capacity is written (d_chain_off and chain.seed_off keep the
 * true offsets).  The seed records from *d_n_seeds up to seed_cap are zeroed (len = 0 breaks the seed rules: the extension
 * answers all -1), so gbx_bsw_extend_seeds_device can follow on the stream for seed_cap seeds without the count.  There are
 * never more seeds than hits: seed_cap = pos_cap always suffices.  work: gbx_mem_chain_workspace_bytes(n_reads, smem_cap,
 * pos_cap) bytes; every read whose hits lie inside pos_cap is chained in full, whatever its hit and chain count. */
size_t gbx_mem_chain_workspace_bytes(int64_t n_reads, int64_t smem_cap, int64_t pos_cap);
int gbx_mem_chain_device(const gbx_mem_chain_params *p, int64_t n_reads,
                         const gbx_fmi_smem *d_smems, const int64_t *d_n_smem, int64_t smem_cap, const int64_t *d_smem_off,
                         const int64_t *d_pos, const int64_t *d_n_pos, int64_t pos_cap, const int64_t *d_pos_off,
                         const int64_t *d_read_off, const int32_t *d_read_len,
                         int64_t l_pac, int32_t n_contigs, const int64_t *d_contig_off,
                         gbx_mem_chain *d_chains, int64_t chain_cap, int64_t *d_chain_off,
                         gbx_bsw_seed *d_seeds, int64_t seed_cap, int32_t *d_l_rep, int64_t *d_n_chains, int64_t *d_n_seeds,
                         void *d_work, size_t work_bytes, void *stream);

/* Host-buffer entry.  Checked before a device is touched: the parameters (w >= 0, e_del and e_ins >= 1), smem_off and
 * pos_off (monotone, inside n_smem / n_pos), read_len >= 0, the contig table.  *n_chains / *n_seeds = the counts; one above
 * its capacity gives GBX_ERR_ARG with the needed counts there and in gbx_last_error() (chains and seeds are then not
 * written; chain_off and l_rep are).  chain_off (n_reads + 1) and l_rep (n_reads) are nullable.  Safe under concurrent host
 * threads; one device. */
int gbx_mem_chain_host(const gbx_mem_chain_params *p, int64_t n_reads,
                       const gbx_fmi_smem *smems, int64_t n_smem, const int64_t *smem_off,
                       const int64_t *pos, int64_t n_pos, const int64_t *pos_off,
                       const int64_t *read_off, const int32_t *read_len,
                       int64_t l_pac, int32_t n_contigs, const int64_t *contig_off,
                       gbx_mem_chain *chains, int64_t chain_cap, int64_t *chain_off,
                       gbx_bsw_seed *seeds, int64_t seed_cap, int32_t *l_rep, int64_t *n_chains, int64_t *n_seeds);

/* ---- CIGAR, edit distance and position of extended seeds (bwa-mem's mem_reg2aln / bwa_gen_cigar2 / ksw_global2: the banded
 * global alignment behind gbx_bsw_extend_seeds_*).  UNPINNED by a compiled reference (bwa's source is not part of the
 * reference tree): the rules are restated in full in DESIGN 3.11 and tests/mem_cigar_ref.py, and pinned by that restatement.
 * Record k: seed s = seeds[k], result r = res[k]; read = qer[s.qoff .. s.qoff + s.lq), the region is query [r.qb, r.qe) against
 * text [s.roff + r.rb, s.roff + r.re) of the 2 L-byte text (L = l_pac, forward strand [0, L)).  Base codes above 4 count as 4.
 *   invalid   r.qb < 0, qe <= qb, rb >= re, rb < L < re, or a range outside its arena (the text ends at min(text_bytes, 2 L)):
 *             rid = -1, n_cigar = 0, every other field 0, no CIGAR words
 *   band      w2 = max(infer_bw(del), infer_bw(ins)) from the region's lengths and r.truesc; above p.w it is cut to r.w
 *   tries     up to three global alignments with the band min(w2, 4 w), doubled while the score stays below r.truesc - a and
 *             changes; the last try's CIGAR and score are kept.  w = the band of the last try, tries = their number
 *   strand    a region at or above L is aligned reversed (query and text), so that indels land leftmost on the forward
 *             strand; the CIGAR is left in that order
 *   global    ksw_global2's recurrence and tie-breaks, gaps opened from the diagonal arrival; equal lengths under a band of 0
 *             are one M run without a DP
 *   nm        mismatching M positions + inserted bases + deleted bases of every D that is neither the first nor the last op
 *   position  p = rb, or 2 L - re on the reverse strand; a leading D is removed and added to p, otherwise a trailing D is
 *             removed; rid / pos from the contig table; soft clips (S) for the read's bases outside [qb, qe)
 * CIGAR words are len << 4 | op with BAM's numbers (M 0, I 1, D 2, S 4), as gbx_pileup_reads takes them.
 * Every valid record it is handed is aligned: the choice of regions, sub, mapq and the supplementary flag are made by
 * gbx_mem_regs_* (below), whose CIGAR list is the input meant for this stage.  Not modelled: the MD string, alt contigs,
 * hard clips. */
typedef struct gbx_mem_cigar_params {    /* 120 bytes */
    int32_t mat[25];                 /* 5 x 5, mat[t * 5 + q]; a = mat[0].  bwa: 1 / -4 / -1 (N) */
    int32_t o_del, e_del, o_ins, e_ins;  /* 6, 1, 6, 1 */
    int32_t w;                       /* 100 */
} gbx_mem_cigar_params;
void gbx_mem_cigar_default_params(gbx_mem_cigar_params *p);

typedef struct gbx_mem_aln {         /* 48 bytes */
    int64_t pos;                     /* 0-based, forward strand, inside contig rid */
    int64_t cigar_off;               /* its words are cigar[cigar_off .. cigar_off + n_cigar) */
    int32_t rid;                     /* contig; -1 invalid record, -2 no room for its direction bytes (device entry only) */
    int32_t is_rev, n_cigar, nm;
    int32_t score;                   /* of the global alignment */
    int32_t w, tries, pad_;
} gbx_mem_aln;

/* Direction bytes one record of query length lq and text length lt can need at most (its band at its widest, 4 w).  The
 * device entry gives every record, in index order, the room its own band asks for (never more than this); a caller sizes
 * z_bytes as the number of regions it expects times this value for its longest read and window, or, knowing nothing, grows
 * z_bytes and repeats the call while records come back with rid = -2. */
size_t gbx_mem_cigar_record_z_bytes(const gbx_mem_cigar_params *p, int32_t lq, int32_t lt);

/* Device entry.  All pointers are device pointers; asynchronous on `stream`, no host synchronisation inside.  n may be the
 * seed_cap of the extension before it on the stream: the zeroed seeds past the count have results of all -1 and give invalid
 * records.  d_text / d_qer: the arenas of gbx_bsw_extend_seeds_device.  Written: d_alns[n], d_cigar[cigar_cap], *d_n_cigar.
 * alns[k].cigar_off and *d_n_cigar are always the true values; nothing past cigar_cap is written.  work:
 * gbx_mem_cigar_workspace_bytes(n, z_bytes) bytes, z_bytes of them the direction room; a record whose room ends past z_bytes
 * gets rid = -2, n_cigar = 0 (the records after it that still fit are aligned).  The output bytes do not depend on the
 * scheduling. */
size_t gbx_mem_cigar_workspace_bytes(int64_t n, int64_t z_bytes);
int gbx_mem_cigar_device(const gbx_mem_cigar_params *p, int64_t n,
                         const gbx_bsw_seed *d_seeds, const gbx_bsw_seed_result *d_res,
                         const uint8_t *d_text, int64_t text_bytes, const uint8_t *d_qer, int64_t qer_bytes,
                         int64_t l_pac, int32_t n_contigs, const int64_t *d_contig_off,
                         gbx_mem_aln *d_alns, uint32_t *d_cigar, int64_t cigar_cap, int64_t *d_n_cigar,
                         void *d_work, size_t work_bytes, void *stream);

/* Host-buffer entry.  Checked before a device is touched: the parameters (w >= 0, e_del and e_ins >= 1), the contig table,
 * and every record that is not the extension's all -1 answer: its read and its region inside the arenas (GBX_ERR_ARG naming
 * the lowest bad record).  The direction room is sized exactly, so rid = -2 does not occur.  *n_cigar = the word count; more
 * than cigar_cap gives GBX_ERR_ARG with the need there and in gbx_last_error() (alns are written, cigar is not).  Safe under
 * concurrent host threads; one device. */
int gbx_mem_cigar_host(const gbx_mem_cigar_params *p, int64_t n,
                       const gbx_bsw_seed *seeds, const gbx_bsw_seed_result *res,
                       const uint8_t *text, int64_t text_bytes, const uint8_t *qer, int64_t qer_bytes,
                       int64_t l_pac, int32_t n_contigs, const int64_t *contig_off,
                       gbx_mem_aln *alns, uint32_t *cigar, int64_t cigar_cap, int64_t *n_cigar);

/* ---- alignment regions, primary marking and mapping quality (bwa-mem's redundancy skip of mem_chain2aln, mem_sort_dedup_patch,
 * mem_mark_primary_se, mem_approx_mapq_se and the region choice of mem_reg2sam: the step between gbx_bsw_extend_seeds_* and
 * gbx_mem_cigar_*).  UNPINNED by a compiled reference (bwa's source is not part of the reference tree): the rules are restated
 * in full in DESIGN 3.12 and tests/mem_regs_ref.py, and pinned by that restatement.
 * Read r owns chains[chain_off[r] .. chain_off[r+1]); seed k of a chain is seeds[seed_off + k] with the result res[seed_off + k];
 * absolute coordinates are s.roff + s.rbeg and s.roff + res.rb / res.re.  A seed whose result has qb < 0 is absent.
 *   seeds     per chain by (len, index) from the largest down; a seed inside an earlier region of the read on both axes, not
 *             longer than its seedlen0 by more than .1 lq and within min(gap, region.w) of its diagonal ahead or behind, makes
 *             no region unless a taken seed t of the chain (t.len >= .95 s.len) overlaps it by s.len >> 2 query bases off its
 *             diagonal; a taken seed's region is its extension result, seedlen0 = len, rid = the chain's contig, seedcov = the
 *             length of the chain's seeds inside the region
 *   dedup     by (re, creation): of two regions of one contig within max_chain_gap that overlap by more than mask_level_redun
 *             (fp32) of the shorter on both axes the lower score goes (the earlier one on a tie); then by (score desc, rb, qb):
 *             a region equal to its predecessor in all three goes.  mem_patch_reg (the merge of two collinear regions) and
 *             n_comp are NOT modelled
 *   primary   by (score desc, hash_64(read_id0 + r + i), i): a region overlapping an earlier primary by mask_level (fp32) of the
 *             shorter query span is secondary to it, sets its sub once and counts in its sub_n within max(a + b, o_del + e_del,
 *             o_ins + e_ins); this is the output order
 *   mapq      mem_approx_mapq_se: sub = max(sub ? sub : min_seed_len * a, csub), csub = 0 in every region this stage makes, and
 *             frac_rep = (float)l_rep[r] / lq (0 for a region with seedlen0 == 0: a rescued one); 0 for a secondary.  A region of
 *             length 0 gets 0
 *   report    score >= T and not secondary; the second and later reported regions of a read are supplementary (0x800) and
 *             their mapq is capped by the first's
 * Not modelled: mem_patch_reg, alt contigs, MEM_F_ALL, XA, bwa's other mapq formula (mapq_coef_len <= 0).  Paired-end reads:
 * gbx_mem_rescue_* and gbx_mem_pair_* below. */
typedef struct gbx_mem_regs_params {     /* 64 bytes */
    int32_t a, b;                        /* 1, 4 */
    int32_t o_del, e_del, o_ins, e_ins;  /* 6, 1, 6, 1 */
    int32_t w;                           /* 100 */
    int32_t max_chain_gap;               /* 10000 */
    int32_t min_seed_len;                /* 19 */
    int32_t T;                           /* 30: regions scoring below it are not reported */
    int32_t mapq_coef_len;               /* 50; must be > 0 (bwa's other mapq formula is not modelled: GBX_ERR_UNSUPPORTED) */
    float   mapq_coef_fac;               /* (float)log((double)mapq_coef_len), set by the host */
    float   mask_level, mask_level_redun, drop_ratio;   /* 0.5, 0.95, 0.5 */
    int32_t pad_;
} gbx_mem_regs_params;
void gbx_mem_regs_default_params(gbx_mem_regs_params *p);

typedef struct gbx_mem_reg {             /* 88 bytes */
    int64_t rb, re;                      /* text coordinates, [0, 2 L) */
    int64_t seed;                        /* index of the seed record this region was extended from */
    int32_t qb, qe, read, rid;           /* read: its index in the call; rid = the chain's contig */
    int32_t score, truesc, sub, sub_n, w, seedcov, seedlen0;
    int32_t secondary;                   /* -1, or the index (within the read's regions) of the region it is secondary to */
    int32_t mapq;                        /* 0 for a secondary region */
    int32_t flag;                        /* bit 0: reported (went to the CIGAR list); 0x800: supplementary */
    int32_t sel;                         /* its index in the CIGAR list, -1 if not reported */
    int32_t csub;                        /* bwa's csub: the SW's second-best score of a rescued region (gbx_mem_rescue_*), else 0 */
} gbx_mem_reg;

/* Device path.  All pointers are device pointers; asynchronous on `stream`, no host synchronisation inside.  The chain and seed
 * counts are read on the device (the d_n_chains / d_n_seeds of gbx_mem_chain_device on the same stream), d_res is the output of
 * gbx_bsw_extend_seeds_device for those seeds, d_l_rep the chaining's.  Written: d_regs[reg_cap] (every read's regions in the
 * output order above), d_reg_off[n_reads + 1], *d_n_regs, and the CIGAR list: for every reported region in output order a copy
 * of its seed record in d_sel_seeds and a result (qb, qe, rb - seed.roff, re - seed.roff, score, truesc, w, sc0 = 0) in
 * d_sel_res - the fields gbx_mem_cigar_* reads - with *d_n_sel their count.  The records from *d_n_sel up to sel_cap are zeroed
 * seeds with results of all -1, so gbx_mem_cigar_device can follow on the stream for sel_cap records without the count.  A read
 * never makes more regions than it has seeds: reg_cap = sel_cap = seed_cap always suffices.  A count above its capacity reports
 * the need: nothing past the capacity is written (d_reg_off and reg.sel keep the true values).  *d_n_chains > chain_cap or
 * *d_n_seeds > seed_cap means the chaining before it overflowed: *d_n_regs = *d_n_sel = -1, d_reg_off all 0, no region is made
 * and the whole CIGAR list is the zeroed tail.  seed_cap below 2^31.  work: gbx_mem_regs_workspace_bytes(n_reads, seed_cap)
 * bytes; every read is done in full whatever its seed and region count.  The output bytes do not depend on the scheduling. */
size_t gbx_mem_regs_workspace_bytes(int64_t n_reads, int64_t seed_cap);
int gbx_mem_regs_device(const gbx_mem_regs_params *p, int64_t n_reads, int64_t read_id0,
                        const gbx_mem_chain *d_chains, const int64_t *d_n_chains, int64_t chain_cap, const int64_t *d_chain_off,
                        const gbx_bsw_seed *d_seeds, const int64_t *d_n_seeds, int64_t seed_cap,
                        const gbx_bsw_seed_result *d_res, const int32_t *d_l_rep,
                        gbx_mem_reg *d_regs, int64_t reg_cap, int64_t *d_reg_off, int64_t *d_n_regs,
                        gbx_bsw_seed *d_sel_seeds, gbx_bsw_seed_result *d_sel_res, int64_t sel_cap, int64_t *d_n_sel,
                        void *d_work, size_t work_bytes, void *stream);

/* Host-buffer entry.  Checked before a device is touched: the parameters (e_del and e_ins >= 1, a >= 1, a + b >= 1, w >= 0,
 * mapq_coef_len > 0: GBX_ERR_UNSUPPORTED otherwise), chain_off (monotone, inside n_chains) and every chain's seed range (inside
 * n_seeds): GBX_ERR_ARG naming the lowest offender.  *n_regs / *n_sel = the counts; one above its capacity gives GBX_ERR_ARG
 * with the needed counts there and in gbx_last_error() (regs and the CIGAR list are then not written; reg_off is).  On success
 * the CIGAR list is written up to sel_cap, tail included.  reg_off (n_reads + 1) is nullable.  Safe under concurrent host
 * threads; one device. */
int gbx_mem_regs_host(const gbx_mem_regs_params *p, int64_t n_reads, int64_t read_id0,
                      const gbx_mem_chain *chains, int64_t n_chains, const int64_t *chain_off,
                      const gbx_bsw_seed *seeds, int64_t n_seeds, const gbx_bsw_seed_result *res, const int32_t *l_rep,
                      gbx_mem_reg *regs, int64_t reg_cap, int64_t *reg_off, int64_t *n_regs,
                      gbx_bsw_seed *sel_seeds, gbx_bsw_seed_result *sel_res, int64_t sel_cap, int64_t *n_sel);

/* ---- paired-end: insert-size estimate, pairing and the pair decision (bwa-mem's mem_pestat, mem_pair and the decision part of
 * mem_sam_pe: the step between gbx_mem_regs_* and gbx_mem_cigar_*.  On the regs stage's output it is `bwa mem -S`; mate rescue is
 * the stage before it, gbx_mem_rescue_* below, whose output has the regs stage's shape).  A region with seedlen0 == 0 (a rescued
 * one) has frac_rep = 0, and the cap on q_se is raw(c.score - c.csub), csub being 0 in the regs stage's regions.
 * UNPINNED by a compiled reference (bwa's source is not part of the reference tree): the rules are restated in full in DESIGN
 * 3.13 and tests/mem_pair_ref.py, and pinned by that restatement.
 * A call of n_pairs pairs is the regs stage's output for 2 n_pairs interleaved reads, read 2p + e being end e of pair p, made
 * with read_id0 = 2 pair_id0 (its hash is then bwa's hash_64((id << 1 | e) + i), so the primary marking stands).  L = l_pac;
 * a_e[i] = region i of end e in that stage's output order.
 *   infer_dir(b1, b2)  r1 = b1 >= L, r2 = b2 >= L, p2 = r1 == r2 ? b2 : 2L - 1 - b2; dist = |p2 - b1|,
 *             dir = (r1 == r2 ? 0 : 1) ^ (p2 > b1 ? 0 : 3)  (0 FF, 1 FR, 2 RF, 3 RR)
 *   estimate  once per call over all its pairs (skipped when the caller gives pes_in).  Per end top = the region first by
 *             (score desc, rb, qb); cal_sub = the largest score among the other regions whose query interval overlaps top's by
 *             e_min - b_max >= min_l * mask_level (fp32), else min_seed_len * a.  A pair is skipped if an end has no region, if
 *             cal_sub > 0.8 * top.score (double) for either end, or if the tops' rid differ; else (dir, is) = infer_dir(top0.rb,
 *             top1.rb) counts in direction dir if 1 <= is <= max_ins.  Per direction with n values sorted: n < 10 fails (the rest
 *             of the record 0); pK = sorted[(int)(K n + .499)], K = .25, .5, .75; low = max((int)(p25 - 2 (p75 - p25) + .499), 1),
 *             high = (int)(p75 + 2 (p75 - p25) + .499); avg = the mean of the values in [low, high], std = sqrt(S / x) over the
 *             same x values; then low / high = (int)(p25 -/+ 3 (p75 - p25) + .499), moved out to (int)(avg -/+ 4 std + .499) where
 *             that lies further out, low at least 1.  All in double, (int) truncating.  Last, a direction that has not failed
 *             with n < 0.05 max_d n_d fails (its numbers stay).  S = the sum over the values v ascending of
 *             (double)c[v] * ((v - avg) * (v - avg)), c[v] = the number of values equal to v, every product and sum rounded on
 *             its own: the one departure from bwa, which adds one value at a time
 *   pairing   per pair with regions at both ends, unless no_pairing.  Keys over all regions of both ends: fwd = rb < L ? rb :
 *             2L - 1 - rb, x = rid << 32 | (fwd - contig_off[rid]), y = score << 32 | i << 2 | (rb >= L) << 1 | e; sorted by
 *             (x, y).  last[4] = -1; for i over the keys, for r = 0, 1: dir = r << 1 | (y_i >> 1 & 1), skipped if pes[dir]
 *             failed; which = r << 1 | ((y_i & 1) ^ 1); for k from last[which] down to 0 with (y_k & 3) == which: dist = x_i -
 *             x_k on the whole keys; dist > high ends the walk, dist < low skips k, else k is a candidate with ns = (dist - avg)
 *             / std, qd = (double)(score_i + score_k) + .721 * log(2. * erfc(fabs(ns) * M_SQRT1_2)) * a + .499, q = qd > 0 ?
 *             (int)qd : 0 (erfc underflows to 0 far out: log gives -inf, q = 0), X = q << 32 | (hash_64(Y ^ (pair_id << 8)) &
 *             0xffffffff), Y = k << 32 | i, pair_id = pair_id0 + p; after both r, last[y_i & 3] = i.  No candidate: score = sub =
 *             n_sub = 0.  Else the best is the largest (X, Y): z[y & 1] = (y & 0xffffffff) >> 2 for its two keys, score = its q,
 *             sub = the second largest's q (0 with one candidate), n_sub = the candidates other than the best with sub - q <=
 *             max(a + b, o_del + e_del, o_ins + e_ins)
 *   decision  mapq_se(reg) = the regs stage's mapq rule on the region's current sub and sub_n, without its secondary test;
 *             raw(d) = (int)(6.02 * d / a + .499).  Paired branch - pairing ran with score > 0 and neither end has a region
 *             j >= 1 with secondary < 0 && score >= T: score_un = a_0[0].score + a_1[0].score - pen_unpaired, subo = max(sub,
 *             score_un), q_pe = raw(score - subo), less (int)(4.343 * log(n_sub + 1) + .499) if n_sub > 0, clamped to [0, 60],
 *             then (int)(q_pe * (1. - .5 * (frac_rep_0 + frac_rep_1)) + .499), frac_rep_e = (float)l_rep / lq and their sum in
 *             fp32.  If score > score_un, for each end c = a_e[z_e]: a secondary c takes sub = a_e[c.secondary].score and
 *             secondary = -2; q_se = mapq_se(c); q_se = q_se > q_pe ? q_se : min(q_pe, q_se + 40); q_se = min(q_se,
 *             raw(c.score)); proper = 1.  Else z = (0, 0), q_se = mapq_se(a_e[0]), proper = 0.  paired = 1; each read reports
 *             exactly z_e: in d_pregs it has flag 1 and mapq = q_se, every other region of the read flag 0 and sel -1.
 *             Otherwise (paired = 0) the regions stay as the regs stage left them; z_e = 0 if a_e[0].score >= T else -1; q_se =
 *             that region's mapq or 0; q_pe = 0; proper = 1 iff !no_pairing, both z_e == 0, equal rid, and infer_dir(a_0[0].rb,
 *             a_1[0].rb) gives a direction that has not failed with low <= dist <= high.  dir / dist of the pair record:
 *             infer_dir of the two z regions' rb, or -1 / 0 if either is missing
 *   list      the new CIGAR list holds the reads in order, each read's reported regions in output order, each record a copy of
 *             the region's record in the regs stage's list (a region that stage did not report is built as it builds them);
 *             sel is renumbered
 * Not modelled: alt contigs, MEM_F_ALL, XA, mem_patch_reg, the MD string, bwa's secondary_all. */
typedef struct gbx_mem_pair_params {     /* 56 bytes */
    int32_t a, b;                        /* 1, 4 */
    int32_t o_del, e_del, o_ins, e_ins;  /* 6, 1, 6, 1 */
    int32_t min_seed_len, T;             /* 19, 30 */
    int32_t pen_unpaired;                /* 17 */
    int32_t max_ins;                     /* 10000; 1 <= max_ins <= 2^20 */
    int32_t mapq_coef_len;               /* 50; must be > 0 (GBX_ERR_UNSUPPORTED otherwise) */
    float   mapq_coef_fac;               /* (float)log((double)mapq_coef_len), set by the host */
    float   mask_level;                  /* 0.5 */
    int32_t no_pairing;                  /* bwa -P: 1 = pairing is skipped, everything goes the unpaired way */
} gbx_mem_pair_params;
void gbx_mem_pair_default_params(gbx_mem_pair_params *p);

typedef struct gbx_mem_pestat {          /* 32 bytes; four per call: FF, FR, RF, RR */
    int32_t low, high, failed, pad_;
    double  avg, std;
} gbx_mem_pestat;

typedef struct gbx_mem_pair {            /* 56 bytes */
    int64_t dist;                        /* of the two reported regions, 0 if either is missing */
    int32_t score, sub, n_sub, n_cand;   /* what the pairing returned (0 when it did not run); n_cand = its candidate pairs */
    int32_t z0, z1;                      /* the region of each end that is reported first (index within the read), -1 none */
    int32_t q_pe, q_se0, q_se1;
    int32_t paired;                      /* 1: the paired branch ran to its end */
    int32_t proper;                      /* SAM 0x2 */
    int32_t dir;                         /* infer_dir of the two reported regions, -1 if either is missing */
} gbx_mem_pair;

/* Device path.  All pointers are device pointers but pes_in; asynchronous on `stream`, no host synchronisation inside.  d_regs,
 * d_reg_off (2 n_pairs + 1), d_n_regs, d_sel_seeds / d_sel_res (sel_cap): the outputs of gbx_mem_regs_device on the same stream;
 * d_seeds (seed_cap records, read for lq through reg.seed) and d_l_rep the chaining's.  The region count is read on the device;
 * the inputs are never written.  pes_in: null, or a host pointer to four records given by the caller (bwa -I), read during the
 * call; no estimate is made then.  Written: d_pes[4], d_pairs[n_pairs], d_pregs (the first *d_n_regs records: a copy of d_regs
 * with the decision's changes and sel renumbered), the new CIGAR list d_psel_seeds / d_psel_res with its count *d_n_psel.  The
 * records from *d_n_psel up to psel_cap are zeroed seeds with results of all -1, so gbx_mem_cigar_device can follow on the stream
 * for psel_cap records.  The list never holds more records than there are regions: psel_cap = reg_cap always suffices (and so does
 * a sel_cap that was the regs stage's seed_cap); a count above psel_cap reports the need, nothing past the capacity
 * is written (reg.sel keeps the true index).  *d_n_regs < 0 or above reg_cap (the stage before overflowed): *d_n_psel = -1,
 * zeroed pairs, every direction failed, the whole CIGAR list the zeroed tail.  reg_cap below 2^30.  work:
 * gbx_mem_pair_workspace_bytes(n_pairs, reg_cap, max_ins) bytes; every pair is done in full whatever its region count.  The
 * output bytes do not depend on the scheduling. */
size_t gbx_mem_pair_workspace_bytes(int64_t n_pairs, int64_t reg_cap, int32_t max_ins);
int gbx_mem_pair_device(const gbx_mem_pair_params *p, int64_t n_pairs, int64_t pair_id0,
                        const gbx_mem_reg *d_regs, const int64_t *d_reg_off, const int64_t *d_n_regs, int64_t reg_cap,
                        const gbx_bsw_seed *d_sel_seeds, const gbx_bsw_seed_result *d_sel_res, int64_t sel_cap,
                        const gbx_bsw_seed *d_seeds, int64_t seed_cap, const int32_t *d_l_rep,
                        int64_t l_pac, int32_t n_contigs, const int64_t *d_contig_off,
                        const gbx_mem_pestat *pes_in, gbx_mem_pestat *d_pes, gbx_mem_pair *d_pairs, gbx_mem_reg *d_pregs,
                        gbx_bsw_seed *d_psel_seeds, gbx_bsw_seed_result *d_psel_res, int64_t psel_cap, int64_t *d_n_psel,
                        void *d_work, size_t work_bytes, void *stream);
/* gbx_mem_pair_device with the caller's estimate on the device: d_pes_in is null (an estimate is made, as with pes_in null) or a
 * DEVICE pointer to four records, e.g. the d_pes of gbx_mem_pestat_device on the same stream; the kernel that fills d_pes reads
 * them, the host never does, so the call chains behind the rescue without a copy or a synchronisation.  The check the other
 * entries make of a caller's records on the host (std > 0 wherever failed == 0) cannot be made here: on the device a record that
 * breaks it is taken as failed (d_pes gets it with failed = 1, its other fields as given).  d_pes_in may be d_pes itself.  Every
 * other argument and every output is that of gbx_mem_pair_device given the same records as pes_in. */
int gbx_mem_pair_device_pes(const gbx_mem_pair_params *p, int64_t n_pairs, int64_t pair_id0,
                            const gbx_mem_reg *d_regs, const int64_t *d_reg_off, const int64_t *d_n_regs, int64_t reg_cap,
                            const gbx_bsw_seed *d_sel_seeds, const gbx_bsw_seed_result *d_sel_res, int64_t sel_cap,
                            const gbx_bsw_seed *d_seeds, int64_t seed_cap, const int32_t *d_l_rep,
                            int64_t l_pac, int32_t n_contigs, const int64_t *d_contig_off,
                            const gbx_mem_pestat *d_pes_in, gbx_mem_pestat *d_pes, gbx_mem_pair *d_pairs, gbx_mem_reg *d_pregs,
                            gbx_bsw_seed *d_psel_seeds, gbx_bsw_seed_result *d_psel_res, int64_t psel_cap, int64_t *d_n_psel,
                            void *d_work, size_t work_bytes, void *stream);

/* Host-buffer entry.  Checked before a device is touched: the parameters (a >= 1, e_del and e_ins >= 1, 1 <= max_ins <= 2^20,
 * mapq_coef_len > 0: GBX_ERR_UNSUPPORTED otherwise), pair_id0 >= 0 and pair_id0 + n_pairs <= 2^23 (beyond it bwa's int id << 8
 * overflows), the contig table, reg_off (monotone, inside n_regs), every reg.rid inside the contig table, every reg.seed inside
 * the seeds, and a caller's pes_in (std > 0 wherever failed == 0): GBX_ERR_ARG naming the lowest offender.  *n_psel = the count;
 * one above psel_cap gives GBX_ERR_ARG with the need there and in gbx_last_error() (pes, pairs and pregs are written, the list
 * is not).  On success the list is written up to psel_cap, tail included.  Safe under concurrent host threads; one device. */
int gbx_mem_pair_host(const gbx_mem_pair_params *p, int64_t n_pairs, int64_t pair_id0,
                      const gbx_mem_reg *regs, const int64_t *reg_off, int64_t n_regs,
                      const gbx_bsw_seed *sel_seeds, const gbx_bsw_seed_result *sel_res, int64_t n_sel,
                      const gbx_bsw_seed *seeds, int64_t n_seeds, const int32_t *l_rep,
                      int64_t l_pac, int32_t n_contigs, const int64_t *contig_off,
                      const gbx_mem_pestat *pes_in, gbx_mem_pestat *pes, gbx_mem_pair *pairs, gbx_mem_reg *pregs,
                      gbx_bsw_seed *psel_seeds, gbx_bsw_seed_result *psel_res, int64_t psel_cap, int64_t *n_psel);

/* ---- the insert-size estimate alone: step `estimate` of the paired-end stage above, from the same kernels.  bwa estimates on the
 * regions before mate rescue, so this runs on the regs stage's output, gbx_mem_rescue_* reads d_pes on the device, and
 * gbx_mem_pair_* behind it is given the same four records as pes_in.  Of p only a, min_seed_len, mask_level and max_ins are
 * read.  d_pes[4] is byte-equal to what gbx_mem_pair_device writes there for the same regions (all four failed after an upstream
 * overflow).  work: gbx_mem_pestat_workspace_bytes(max_ins) bytes.  The host entry checks what gbx_mem_pair_host checks of these
 * arguments. */
size_t gbx_mem_pestat_workspace_bytes(int32_t max_ins);
int gbx_mem_pestat_device(const gbx_mem_pair_params *p, int64_t n_pairs,
                          const gbx_mem_reg *d_regs, const int64_t *d_reg_off, const int64_t *d_n_regs, int64_t reg_cap, int64_t l_pac,
                          gbx_mem_pestat *d_pes, void *d_work, size_t work_bytes, void *stream);
int gbx_mem_pestat_host(const gbx_mem_pair_params *p, int64_t n_pairs, const gbx_mem_reg *regs, const int64_t *reg_off, int64_t n_regs,
                        int64_t l_pac, gbx_mem_pestat *pes);

/* ---- mate rescue (bwa-mem's mem_matesw around ksw_align2: the step between gbx_mem_regs_* and gbx_mem_pair_*).  UNPINNED by a
 * compiled reference (bwa's source is not part of the reference tree): the rules are restated in full in DESIGN 3.14 and
 * tests/mem_rescue_ref.py, and pinned by that restatement, hand-built cases and a frozen example.
 * Input: the regs stage's output for 2 n_pairs interleaved reads and four gbx_mem_pestat records.  Output: the same region lists
 * in the regs stage's shape with the rescued regions added, the lists deduplicated again and primary marking, mapq and the report
 * choice redone, so gbx_mem_pair_* and gbx_mem_cigar_* follow unchanged.  L = l_pac, the text is the 2L-byte text of the other
 * stages, infer_dir as above.
 *   lists     a_e = end e's regions by (score desc, rb, qb); sub, sub_n, secondary, mapq, flag and sel are not read.  b_e = the
 *             regions of a_e with score >= a_e[0].score - pen_unpaired, in order, the first max_matesw; fixed before any rescue
 *   order     for e = 0, 1: for j over b_e: matesw(anchor = b_e[j], mate = the read of end 1 - e, ma = a_{1-e}), strictly serial:
 *             ma carries what earlier calls added or removed
 *   matesw    skip[r] = pes[r].failed; every region m of ma sets skip[r] for (r, dist) = infer_dir(anchor.rb, m.rb) when low_r <=
 *             dist <= high_r; all four set: return.  n = 0; for r = 0 .. 3 not skipped: is_rev = (r >> 1) != (r & 1), is_larger =
 *             !(r >> 1), seq = the mate, reverse-complemented if is_rev (c < 4 ? 3 - c : 4); the window: not is_rev: rb = is_larger
 *             ? anchor.rb + low : anchor.rb - high, re = (is_larger ? anchor.rb + high : anchor.rb - low) + l_ms; is_rev: rb =
 *             (is_larger ? anchor.rb + low : anchor.rb - high) - l_ms, re = is_larger ? anchor.rb + high : anchor.rb - low;
 *             clamped to [0, 2L]; if rb < re it is cut to the contig of (rb + re) >> 1 on that strand, else there is none.  With
 *             a window on the anchor's contig of at least min_seed_len bases: the SW below on seq against text[rb, re), ++n, and
 *             if score >= min_seed_len and qb >= 0 a region B: rid = anchor.rid, (qb, qe) = is_rev ? (l_ms - (qe + 1), l_ms - qb)
 *             : (qb, qe + 1), (rb, re) = is_rev ? (2L - (rb + te + 1), 2L - (rb + tb)) : (rb + tb, rb + te + 1), score, csub =
 *             score2 (-1: none), secondary = -1, seedcov = min(re - rb, qe - qb) >> 1, everything else 0 (truesc, w, seedlen0,
 *             sub, sub_n); B goes in front of the first element of ma with a lower score (behind all without one).  Then, in
 *             the same iteration and whether or not there was a window: if n > 0, ma = dedup(ma) - the regs stage's dedup, ties
 *             of re by the position in ma
 *   SW        ksw_align2 with KSW_XSUBO | KSW_XSTART | min_seed_len * a.  Query q[0, m) along the rows, target t[0, n) along the
 *             columns.  S(x, y) = a if x == y < 4, -b if both < 4 and differ, -1 if either >= 4.  Pw = 16 if m * a < 250 else 8,
 *             slen = ceil(m / Pw); the query is padded to slen * Pw rows with a symbol scoring 0 against everything (bwa's striped
 *             profile): the padded rows take part in the recurrence and the column maxima and never hold the maximum.  H(i, j) =
 *             max(0, H(i-1, j-1) + S, E(i, j), F(i, j)), E(i+1, j) = max(0, E(i, j) - e_del, H(i, j) - o_del - e_del), F(i, j+1) =
 *             max(0, F(i, j) - e_ins, H(i, j) - o_ins - e_ins), 0 outside.  Per column i in order: imax = max_j H(i, j); if imax >=
 *             minsc = min_seed_len * a: with no entry yet or the last entry's column + 1 != i append (imax, i), else a last entry
 *             with a lower value is replaced by (imax, i) (the stored column is that of the run's maximum, not its end); if imax >
 *             gmax: gmax = imax, te = i.  Then score = gmax, qe = the row of column te with H == score that is first in striped
 *             memory order (smallest (j mod slen) * Pw + j div slen), w = (score + a - 1) / a, (score2, te2) = the first entry
 *             in order with the largest value among those whose column lies outside [te - w, te + w], (-1, -1) without one.
 *             score < minsc: qb = tb = -1.  Else the same pass on reverse(q[0, qe]) against reverse(t[0, te]) with the same Pw,
 *             its own slen and padding and no entries, stopping at the first column where gmax >= score, gives (score', te',
 *             qe'); qb = qe - qe', tb = te - te' if score' == score, else both -1.  Not modelled: byte mode's early exit at
 *             gmax + b >= 255 (b > 5 is refused, so it cannot fire)
 *   after     a pair in which no SW ran comes out byte-equal to its input.  Else per read mem_mark_primary_se with read_id = 2
 *             (pair_id0 + p) + e on the final list, then the regs stage's mapq and report rules
 *   records   d_xseeds[0, seed_cap) is a copy of d_seeds; each rescued region that survives gets a record behind it, in output
 *             order: qoff / lq of its read, roff / rlen = its window on the region's own strand ([2L - re, 2L - rb) when is_rev),
 *             qbeg = qb, rbeg = rb - roff, len = 0, and reg.seed points at it.  Its CIGAR-list record is built as the regs stage
 *             builds them, with w = 0 and truesc = 0 as bwa leaves them; gbx_mem_cigar_* retries its band from there
 * Not modelled: alt contigs, MEM_F_ALL, XA, mem_patch_reg, the MD string. */
typedef struct gbx_mem_rescue_params {   /* 64 bytes */
    int32_t a, b;                        /* 1, 4; a <= 63, b <= 5 (GBX_ERR_UNSUPPORTED above) */
    int32_t o_del, e_del, o_ins, e_ins;  /* 6, 1, 6, 1 */
    int32_t min_seed_len, T;             /* 19, 30 */
    int32_t pen_unpaired;                /* 17 */
    int32_t max_matesw;                  /* 50; at least 1 */
    int32_t max_chain_gap;               /* 10000 */
    int32_t mapq_coef_len;               /* 50; must be > 0 */
    float   mapq_coef_fac;               /* (float)log((double)mapq_coef_len), set by the host */
    float   mask_level, mask_level_redun;   /* 0.5, 0.95 */
    int32_t pad_;
} gbx_mem_rescue_params;
void gbx_mem_rescue_default_params(gbx_mem_rescue_params *p);

typedef struct gbx_mem_rescue_stat {     /* 16 bytes, one per pair */
    int32_t n_sw;                        /* SWs whose answer was used (bwa's n, summed over the pair's matesw calls) */
    int32_t n_added;                     /* regions added */
    int32_t n_kept;                      /* rescued regions in the pair's output */
    int32_t pad_;
} gbx_mem_rescue_stat;

/* Device path.  All pointers are device pointers; asynchronous on `stream`, no host synchronisation inside.  d_regs, d_reg_off
 * (2 n_pairs + 1), d_n_regs: the outputs of gbx_mem_regs_device on the same stream, made with read_id0 = 2 pair_id0; d_seeds
 * (seed_cap records) and d_l_rep the chaining's; d_read_off / d_read_len: the reads in d_qer (a mate with no region still has a
 * sequence), reads of 1 .. 1024 bases (a longer mate is not rescued by this entry; the host entry refuses it); d_text: at least
 * 2 l_pac bytes; d_pes: four records on the device (gbx_mem_pestat_device), a direction that has not failed with low < 0, low >
 * high or high > 2^20 gets no window.  The inputs are never written.  Written: d_xregs (every read's regions in output order),
 * d_xreg_off[2 n_pairs + 1], *d_n_xregs; d_xseeds[xseed_cap] with *d_n_xseeds = seed_cap + the surviving rescued regions (the
 * records between that and xseed_cap are zeroed); the CIGAR list d_xsel_seeds / d_xsel_res with *d_n_xsel, its tail zeroed seeds
 * with results of all -1 up to xsel_cap; d_stats[n_pairs].  A pair adds at most 4 regions per anchor: xreg_cap = xsel_cap =
 * reg_cap + 4 min(reg_cap, 2 n_pairs max_matesw) and xseed_cap = seed_cap + 4 min(reg_cap, 2 n_pairs max_matesw) always suffice.
 * A count above its capacity reports the need: nothing past the capacity is written (d_xreg_off, reg.seed and reg.sel keep the
 * true values).  *d_n_regs < 0 or above reg_cap (the stage before overflowed): the three counts are -1, d_xreg_off all 0, zeroed
 * stats, the whole CIGAR list the zeroed tail.  reg_cap and n_pairs below 2^28.  work:
 * gbx_mem_rescue_workspace_bytes(n_pairs, reg_cap, max_matesw) bytes; every pair and every window is done in full whatever its
 * size.  The output bytes do not depend on the scheduling. */
size_t gbx_mem_rescue_workspace_bytes(int64_t n_pairs, int64_t reg_cap, int32_t max_matesw);
int gbx_mem_rescue_device(const gbx_mem_rescue_params *p, int64_t n_pairs, int64_t pair_id0,
                          const gbx_mem_reg *d_regs, const int64_t *d_reg_off, const int64_t *d_n_regs, int64_t reg_cap,
                          const gbx_bsw_seed *d_seeds, int64_t seed_cap, const int32_t *d_l_rep,
                          const int64_t *d_read_off, const int32_t *d_read_len,
                          const uint8_t *d_text, int64_t text_bytes, const uint8_t *d_qer, int64_t qer_bytes,
                          int64_t l_pac, int32_t n_contigs, const int64_t *d_contig_off, const gbx_mem_pestat *d_pes,
                          gbx_mem_reg *d_xregs, int64_t xreg_cap, int64_t *d_xreg_off, int64_t *d_n_xregs,
                          gbx_bsw_seed *d_xseeds, int64_t xseed_cap, int64_t *d_n_xseeds,
                          gbx_bsw_seed *d_xsel_seeds, gbx_bsw_seed_result *d_xsel_res, int64_t xsel_cap, int64_t *d_n_xsel,
                          gbx_mem_rescue_stat *d_stats, void *d_work, size_t work_bytes, void *stream);

/* Host-buffer entry.  Checked before a device is touched: the parameters (a >= 1, e_del and e_ins >= 1, o_del and o_ins >= 0,
 * max_matesw >= 1, mapq_coef_len > 0; a > 63 or b > 5: GBX_ERR_UNSUPPORTED), pair ids as in gbx_mem_pair_host, the contig table,
 * text_bytes >= 2 l_pac, reg_off, every reg.rid and reg.seed, every read inside qer with 1 .. 1024 bases (longer:
 * GBX_ERR_UNSUPPORTED), and pes: 0 <= low <= high <= 2^20 wherever a direction has not failed: GBX_ERR_ARG naming the lowest
 * offender.  The counts go to *n_xregs, *n_xseeds, *n_xsel; one above its capacity gives GBX_ERR_ARG with the need there and in
 * gbx_last_error() (xreg_off and stats are written, the lists are not).  Safe under concurrent host threads; one device. */
int gbx_mem_rescue_host(const gbx_mem_rescue_params *p, int64_t n_pairs, int64_t pair_id0,
                        const gbx_mem_reg *regs, const int64_t *reg_off, int64_t n_regs,
                        const gbx_bsw_seed *seeds, int64_t n_seeds, const int32_t *l_rep,
                        const int64_t *read_off, const int32_t *read_len,
                        const uint8_t *text, int64_t text_bytes, const uint8_t *qer, int64_t qer_bytes,
                        int64_t l_pac, int32_t n_contigs, const int64_t *contig_off, const gbx_mem_pestat *pes,
                        gbx_mem_reg *xregs, int64_t xreg_cap, int64_t *xreg_off, int64_t *n_xregs,
                        gbx_bsw_seed *xseeds, int64_t xseed_cap, int64_t *n_xseeds,
                        gbx_bsw_seed *xsel_seeds, gbx_bsw_seed_result *xsel_res, int64_t xsel_cap, int64_t *n_xsel,
                        gbx_mem_rescue_stat *stats);

/* ---- SAM records (bwa-mem's mem_aln2sam and add_cigar, the MD part of bwa_gen_cigar2: the step behind gbx_mem_cigar_*).
 * UNPINNED by a compiled reference (bwa's source is not part of the reference tree): the rules are restated in full in DESIGN
 * 3.15 and tests/mem_sam_ref.py, and pinned by that restatement, hand-built cases with their lines written out and a frozen
 * example.  L = l_pac; positions are printed 1-based, numbers in decimal.
 * Input: mode 0: n_reads single-end reads with the regs stage's regions and the CIGAR stage's answer for its list; mode 1:
 * n_reads = 2 n_pairs interleaved reads with the paired stage's pairs, pregs and the answer for its list.  reg.sel indexes alns.
 *   records   read r's list: its regions with flag & 1 and sel inside alns, in order; record k (which = k) has rid, pos, is_rev, nm
 *             and the CIGAR words of alns[reg.sel], mapq = reg.mapq, as_ = reg.score, xs = max(reg.sub, reg.csub), 0x800 from
 *             reg.flag.  An empty list gives one unmapped record: rid = pos = -1, flag 0x4, mapq 0, no CIGAR, as_ = xs = 0.  An
 *             aln with rid outside the contigs makes its record unmapped (the host entry refuses it).  0x100 never occurs
 *   mate      mode 1: m = the first record of the other end's list if it is mapped, else none.  flag: 0x1, 0x40 / 0x80 by end, 0x2
 *             from pairs[r >> 1].proper, 0x4 unmapped, 0x8 no m.  An unmapped record takes m's rid, pos and strand (no CIGAR);
 *             without m a mapped record's own rid, pos and strand stand for the mate's.  Then 0x10 from the record's strand and
 *             0x20 from the mate's.  mrid / mpos = those, -1 when there are none.  tlen = -(p0 - p1 + sign(p0 - p1)), pX = pos +
 *             (is_rev ? reference length of the CIGAR - 1 : 0), when the record and m have CIGARs on one contig, else 0.  Mode 0:
 *             only 0x4, 0x10 and 0x800, mrid = mpos = -1
 *   CIGAR     the words as <len><op> with M I D S (any other op counts as S); with softclip == 0 and which > 0 every S prints as H;
 *             a record with a position and no words prints *
 *   SEQ       [sq_b, sq_e) of the stored read: [0, lq), less the first and the last clip when they print as H (forward: the
 *             first clip from the start; reverse: the first clip from the end).  Forward: ACGTN; reverse: the range backwards as
 *             TGCAN, QUAL backwards.  An unmapped record on a reverse mate's strand is printed reversed.  QUAL bytes are copied as
 *             they are; * without a quality arena
 *   tags      NM:i: and MD:Z: with a CIGAR; MC:Z: when m has a CIGAR (m's words, S as H by THIS record's which: bwa's
 *             behaviour); AS:i: if as_ >= 0; XS:i: if xs >= 0; SA:Z: for a mapped record whose read has other mapped records
 *             (n_sa of them), each in list order as name,pos+1,+|-,CIGAR with S kept,mapq,NM;
 *   MD        the CIGAR over the read as SEQ prints it before any hard clip against the forward text from contig_off[rid] + pos
 *             (codes above 4 count as 4, 4 equals 4): an M position that differs emits the run count and the reference base; I
 *             and clips advance the read; a D that is neither the first nor the last op that is no clip emits the count, ^ and
 *             its bases and resets the count, a first or last D only advances; the final count ends the string
 *   line      QNAME FLAG RNAME POS MAPQ CIGAR RNEXT PNEXT TLEN SEQ QUAL and the tags, tab-separated, \n-terminated; a record
 *             without a position prints * 0 0 * for RNAME .. CIGAR, one without a mate position * 0 0 for RNEXT .. TLEN.  Lines
 *             go read by read, a read's records in list order
 * Not built: RG, XA, pa, comments, MEM_F_ALL, alt contigs, BAM. */
typedef struct gbx_mem_sam_params {      /* 8 bytes */
    int32_t softclip;                    /* bwa -Y: 0 (supplementary records are hard-clipped) or 1 */
    int32_t pad_;
} gbx_mem_sam_params;
void gbx_mem_sam_default_params(gbx_mem_sam_params *p);

typedef struct gbx_mem_sam_rec {         /* 112 bytes; a record and its line carry the same values */
    int64_t pos, mpos;                   /* 0-based, -1: none */
    int64_t tlen;
    int64_t cigar_off;                   /* its words are cigar[cigar_off .. cigar_off + n_cigar) of the input */
    int64_t md_off;                      /* its MD string is md[md_off .. md_off + md_len) */
    int64_t line_off;                    /* its line is lines[line_off .. line_off + line_len), the \n included */
    int32_t read, which;                 /* the read's index in the call; the record's index in the read's list */
    int32_t flag, rid, mapq, mrid;
    int32_t nm, as_, xs;
    int32_t n_cigar, md_len;
    int32_t sq_b, sq_e;                  /* SEQ and QUAL print [sq_b, sq_e) of the stored read */
    int32_t line_len;
    int32_t n_sa;                        /* entries of its SA tag */
    int32_t pad_;
} gbx_mem_sam_rec;

/* A text_cap (and md_cap) that suffices when the call makes at most rec_cap records, no read has more than max_recs of them, no
 * record deletes more than max_del bases, and the reads, their names and the CIGAR words take read_bytes, name_bytes and
 * cigar_words in all; max_contig_name: the longest contig name. */
size_t gbx_mem_sam_text_cap(int64_t rec_cap, int64_t cigar_words, int64_t read_bytes, int64_t name_bytes, int32_t max_contig_name,
                            int32_t max_recs, int32_t max_del);

/* Device entry.  All pointers are device pointers; asynchronous on `stream`, no host synchronisation inside.  d_regs, d_reg_off
 * (n_reads + 1), d_n_regs: the regs stage's (mode 0) or the rescue / regs stage's reg_off and count with the paired stage's
 * pregs (mode 1; d_pairs: n_reads / 2 records, null in mode 0); d_alns (n_alns records), d_cigar, d_n_cigar: the CIGAR stage's
 * answer for that stage's list; d_qer / d_read_off / d_read_len: the reads as gbx_mem_rescue_device takes them; d_qual: null, or
 * the quality bytes at the same offsets; d_names / d_name_off (n_reads + 1) and d_cnames / d_cname_off (n_contigs + 1): the
 * names as byte arenas; d_text: at least 2 l_pac bytes.  The inputs are never written.  Written: d_recs in line order,
 * d_rec_off[n_reads + 1], *d_n_recs; d_md with *d_n_md; d_lines with *d_n_text.  n_reads + min(reg_cap, n_alns) records always
 * suffice.  A count above its capacity reports the need: nothing past the capacity is written, and the offsets in the records
 * that are written keep the true values.  *d_n_regs < 0 or above reg_cap (the stage before overflowed): the three counts are -1
 * and d_rec_off, d_recs, d_md and d_lines are zeroed.  A malformed input (offsets outside an arena, words outside d_cigar, a
 * CIGAR longer than its read or running off its contig) is cut to what is there and never read past.  work:
 * gbx_mem_sam_workspace_bytes(n_reads, reg_cap, n_alns) bytes.  The output bytes do not depend on the scheduling. */
size_t gbx_mem_sam_workspace_bytes(int64_t n_reads, int64_t reg_cap, int64_t n_alns);
int gbx_mem_sam_device(const gbx_mem_sam_params *p, int64_t n_reads, int32_t mode,
                       const gbx_mem_reg *d_regs, const int64_t *d_reg_off, const int64_t *d_n_regs, int64_t reg_cap,
                       const gbx_mem_pair *d_pairs,
                       const gbx_mem_aln *d_alns, int64_t n_alns, const uint32_t *d_cigar, const int64_t *d_n_cigar, int64_t cigar_cap,
                       const uint8_t *d_qer, int64_t qer_bytes, const int64_t *d_read_off, const int32_t *d_read_len, const uint8_t *d_qual,
                       const uint8_t *d_names, const int64_t *d_name_off, int64_t name_bytes,
                       const uint8_t *d_cnames, const int64_t *d_cname_off, int64_t cname_bytes,
                       const uint8_t *d_text, int64_t text_bytes, int64_t l_pac, int32_t n_contigs, const int64_t *d_contig_off,
                       gbx_mem_sam_rec *d_recs, int64_t rec_cap, int64_t *d_rec_off, int64_t *d_n_recs,
                       uint8_t *d_md, int64_t md_cap, int64_t *d_n_md, uint8_t *d_lines, int64_t text_cap, int64_t *d_n_text,
                       void *d_work, size_t work_bytes, void *stream);

/* Host-buffer entry.  Checked before a device is touched: softclip (0 or 1), mode (0 or 1; n_reads even in mode 1), the contig
 * table, text_bytes >= 2 l_pac, reg_off, name_off and cname_off (monotone, inside their arenas), every read inside qer with at
 * least one base, and every reported region: reg.sel inside alns, its aln's rid inside the contigs, its words inside cigar with
 * ops M I D S only, covering the read exactly and staying on the contig: GBX_ERR_ARG naming the lowest offender.  The counts go
 * to *n_recs, *n_md and *n_text; one above its capacity gives GBX_ERR_ARG with the need there and in gbx_last_error() (rec_off is
 * written; recs, md and lines are not).  Safe under concurrent host threads; one device. */
int gbx_mem_sam_host(const gbx_mem_sam_params *p, int64_t n_reads, int32_t mode,
                     const gbx_mem_reg *regs, const int64_t *reg_off, int64_t n_regs, const gbx_mem_pair *pairs,
                     const gbx_mem_aln *alns, int64_t n_alns, const uint32_t *cigar, int64_t n_cigar,
                     const uint8_t *qer, int64_t qer_bytes, const int64_t *read_off, const int32_t *read_len, const uint8_t *qual,
                     const uint8_t *names, const int64_t *name_off, int64_t name_bytes,
                     const uint8_t *cnames, const int64_t *cname_off, int64_t cname_bytes,
                     const uint8_t *text, int64_t text_bytes, int64_t l_pac, int32_t n_contigs, const int64_t *contig_off,
                     gbx_mem_sam_rec *recs, int64_t rec_cap, int64_t *rec_off, int64_t *n_recs,
                     uint8_t *md, int64_t md_cap, int64_t *n_md, uint8_t *lines, int64_t text_cap, int64_t *n_text);

/* ---- the whole path in one call: reads in, SAM out.  A gbx_mem_aligner queues smem -> sal -> chain -> extend -> regs ->
 * [pestat -> rescue ->] pair -> cigar -> sam (mode 1, interleaved pairs) or smem -> sal -> chain -> extend -> regs -> cigar -> sam
 * (mode 0, single-end) on a stream of its own, exactly as the stage entries above chain, with no host synchronisation between
 * the stages: behind the chain one kernel gathers every stage's count into a gbx_mem_align_counts record, that record is copied
 * and the stream synchronised once, and only then exactly n_recs records and n_text bytes come back.  A capacity that was too
 * small makes the aligner grow it to the reported need and queue the chain again from the first stage that overflowed; what
 * lies before that stage is kept.  The sam and recs bytes of a run depend only on the index, the parameters, the reads and id0:
 * not on the first capacities, the reruns, what the aligner ran before, or the scheduling.
 * Not built: multi-device spreading, alt contigs, XA, mem_patch_reg, RG, BAM, @PG. */
typedef struct gbx_mem_index gbx_mem_index;         /* the device copies of an index; read-only once made, shareable */
typedef struct gbx_mem_aligner gbx_mem_aligner;     /* one stream, all stage buffers, pinned in / out buffers; one thread at a time */

typedef struct gbx_mem_align_params {    /* 600 bytes */
    gbx_fmi_params fmi;
    gbx_mem_chain_params chain;
    gbx_bsw_seed_params bsw;
    gbx_mem_regs_params regs;
    gbx_mem_pair_params pair;            /* also the estimate's (gbx_mem_pestat_*) */
    gbx_mem_rescue_params rescue;
    gbx_mem_cigar_params cigar;
    gbx_mem_sam_params sam;
    int32_t max_occ;                     /* 500: the suffix-array lookup's; equals chain.max_occ */
    int32_t mode;                        /* 0 single-end, 1 interleaved pairs (read 2p + e is end e of pair p) */
    int32_t have_pes;                    /* 1: pes below is the estimate (bwa -I); none is made */
    int32_t no_rescue;                   /* 1: mode 1 without pestat and rescue (bwa -S): regs, pair, cigar, sam */
    gbx_mem_pestat pes[4];
} gbx_mem_align_params;
/* every stage's own defaults, max_occ 500, mode 1 */
void gbx_mem_align_default_params(gbx_mem_align_params *p);
/* Writes every copy of these values the stage structs hold: a / b into the chain's a, the bsw and cigar matrices (bwa_fill_scmat,
 * N scoring -1), regs, pair and rescue; the gap costs into chain, bsw, regs, pair, rescue and cigar; w into chain, bsw, regs and
 * cigar; zdrop and the clip bonuses into bsw; pen_unpaired into pair and rescue; T into regs, pair and rescue; min_seed_len into
 * fmi (with split_len = (int)(min_seed_len * 1.5 + .499)), chain, regs, pair and rescue. */
void gbx_mem_align_set_scoring(gbx_mem_align_params *p, int32_t a, int32_t b, int32_t o_del, int32_t e_del, int32_t o_ins, int32_t e_ins,
                               int32_t pen_clip5, int32_t pen_clip3, int32_t pen_unpaired, int32_t w, int32_t zdrop, int32_t min_seed_len,
                               int32_t T);
/* Host only.  GBX_ERR_ARG naming the first pair of copies that disagree (the fields above, max_chain_gap, mask_level,
 * mask_level_redun, drop_ratio, mapq_coef_len / _fac, max_occ), a mode or flag that is not 0 or 1, or a given pes that breaks
 * std > 0 where failed == 0.  gbx_mem_aligner_create makes it. */
int gbx_mem_align_check_params(const gbx_mem_align_params *p);

typedef struct gbx_mem_align_caps {      /* 128 bytes: every capacity of the chain, in stage order */
    int64_t slot;                        /* fmi: records per read slot; 0 = the stage's own max(48, 4 max_read_len / min_seed_len + 16) */
    int64_t out_cap, pos_cap, chain_cap, seed_cap, reg_cap, sel_cap;
    int64_t xreg_cap, xseed_cap, xsel_cap;       /* the rescue's; 0 where it does not run */
    int64_t psel_cap;                    /* 0 in mode 0 */
    int64_t cigar_cap, z_bytes;
    int64_t rec_cap, md_cap, text_cap;
} gbx_mem_align_caps;
typedef struct gbx_mem_align_counts {    /* 144 bytes: what the gather kernel reads behind the chain; -1: a stage before it overflowed */
    int64_t slot_worst;                  /* gbx_fmi_overflow's word: 0, or a lower bound of the slot a read asked for */
    int64_t n_smem, n_pos, n_chains, n_seeds, n_regs, n_sel;
    int64_t n_xregs, n_xseeds, n_xsel;   /* 0 where the rescue does not run */
    int64_t n_psel;                      /* 0 in mode 0 */
    int64_t n_cigar;
    int64_t n_z_miss;                    /* CIGAR records with rid == -2: no room for their direction bytes */
    int64_t n_recs, n_md, n_text;
    int64_t n_alns;                      /* CIGAR records that were aligned (rid >= 0) */
    int64_t pad_;
} gbx_mem_align_counts;
#define GBX_MEM_ALIGN_MAX_RERUNS 64
/* the stages as rerun_stage names them */
#define GBX_MEM_ST_SMEM 0
#define GBX_MEM_ST_SAL 1
#define GBX_MEM_ST_CHAIN 2
#define GBX_MEM_ST_EXTEND 3
#define GBX_MEM_ST_REGS 4
#define GBX_MEM_ST_PESTAT 5
#define GBX_MEM_ST_RESCUE 6
#define GBX_MEM_ST_PAIR 7
#define GBX_MEM_ST_CIGAR 8
#define GBX_MEM_ST_SAM 9
typedef struct gbx_mem_align_stats {
    gbx_mem_align_counts counts;         /* the last pass's */
    gbx_mem_align_caps caps;             /* in force at the end of the run */
    int64_t runs;                        /* runs of this aligner that reached the device, this one included */
    int64_t bytes_up, bytes_down;        /* moved over the bus by this run */
    int32_t reruns;                      /* passes after the first */
    int32_t slot_reruns;                 /* those the fmi slot started */
    int32_t rerun_stage[GBX_MEM_ALIGN_MAX_RERUNS];   /* the stage each rerun started from; the first GBX_MEM_ALIGN_MAX_RERUNS */
} gbx_mem_align_stats;
/* Per-stage device times: gbx_profile_begin / gbx_profile_end around a run name every stage's kernels. */
typedef struct gbx_mem_align_out {
    const uint8_t *sam; int64_t n_text;  /* the lines, no header */
    const gbx_mem_sam_rec *recs; int64_t n_recs;
    const int64_t *rec_off;              /* n_reads + 1 */
    gbx_mem_pestat pes[4];               /* the estimate in force (all failed where none is made: mode 0) */
    gbx_mem_align_stats stats;
} gbx_mem_align_out;

/* sizeof of params, caps, counts, stats, out, in that order: a binding checks its mirror against it */
void gbx_mem_align_sizes(int64_t out[5]);

/* Host only, no device.  Capacities for a batch of n_reads reads of `bases` bases in all, the longest max_read_len, their names
 * name_bytes.  Where the header states a relation that always suffices and costs nothing it is used: seed_cap = pos_cap, reg_cap =
 * sel_cap = seed_cap, the rescue's three from reg_cap and max_matesw, psel_cap = the rescue's xreg_cap (reg_cap without it),
 * rec_cap = n_reads + min(reg_cap', list length), md_cap = text_cap = gbx_mem_sam_text_cap(rec_cap, cigar_cap, bases, name_bytes,
 * 32, 4, 256).  out_cap, pos_cap, chain_cap, cigar_cap and z_bytes have no such bound: a first guess per base or per read, or,
 * with `last` (the counts of an earlier batch of last_bases bases), those counts scaled by bases / last_bases with a margin of
 * one quarter; never less than the scaled count. */
int gbx_mem_align_plan(const gbx_mem_align_params *p, int64_t n_reads, int64_t bases, int32_t max_read_len, int64_t name_bytes,
                       const gbx_mem_align_counts *last, int64_t last_bases, gbx_mem_align_caps *caps);

/* Uploads and lays out everything once: the index (gbx_fmi_index_build), the samples (gbx_fmi_sa_build), the 2 l_pac-byte text,
 * the contig table and names.  idx->cp_occ, sa->ms_byte, sa->ls_word, text, contig_off, cnames, cname_off: HOST pointers. */
int gbx_mem_index_create(const gbx_fmi_index *idx, const gbx_fmi_sa *sa, const uint8_t *text, int64_t l_pac, int32_t n_contigs,
                         const int64_t *contig_off, const uint8_t *cnames, const int64_t *cname_off, gbx_mem_index **out);
/* The same index from the genome alone (host pointers): built on the device with sa_compx 3 (gbx_fmi_build_device) and handed to
 * the same layout passes, so nothing of the index crosses to the host.  Limits and checks as gbx_fmi_build_host and
 * gbx_mem_index_create. */
int gbx_mem_index_build(const uint8_t *genome, int64_t l_pac, int32_t n_contigs, const int64_t *contig_off,
                        const uint8_t *cnames, const int64_t *cname_off, gbx_mem_index **out);
void gbx_mem_index_destroy(gbx_mem_index *index);
/* The @SQ lines, one per contig.  *need = their bytes; GBX_ERR_ARG when cap is less (nothing is written). */
int gbx_mem_sam_header(const gbx_mem_index *index, uint8_t *buf, int64_t cap, int64_t *need);

/* first: the capacities to start from (null: gbx_mem_align_plan's for the first batch).  The index must outlive the aligner. */
int gbx_mem_aligner_create(const gbx_mem_index *index, const gbx_mem_align_params *p, const gbx_mem_align_caps *first, gbx_mem_aligner **out);
void gbx_mem_aligner_destroy(gbx_mem_aligner *al);
/* Synchronous.  Reads as base codes 0..4, read r = enc[read_off[r] ..+ read_len[r]); qual: null, or bytes at the same offsets;
 * names / name_off (n_reads + 1): the QNAMEs.  Mode 1: n_reads even, id0 the first PAIR's id (the stages get pair_id0 = id0,
 * read_id0 = 2 id0); mode 0: id0 the first read's id.  Checked before any device work, GBX_ERR_ARG naming the lowest offender:
 * n_reads even in mode 1, read_off / name_off monotone and inside their arenas, every read at least one base and inside enc,
 * id0 >= 0 and id0 + n_pairs <= 2^23 (mode 0: id0 + n_reads <= 2^24); GBX_ERR_UNSUPPORTED: a read longer than GBX_BSW_MAX_QLEN,
 * or than 1024 where the rescue runs.  out's pointers are pinned host memory of the aligner, valid until its next run or its
 * destruction.  A failed run leaves stats.runs as it was unless device work had begun. */
int gbx_mem_aligner_run(gbx_mem_aligner *al, int64_t n_reads, int64_t id0, const uint8_t *enc, int64_t enc_bytes,
                        const int64_t *read_off, const int32_t *read_len, const uint8_t *qual,
                        const uint8_t *names, const int64_t *name_off, gbx_mem_align_out *out);
/* The stats of the last run (the run counter also after a refused one). */
int gbx_mem_aligner_stats(const gbx_mem_aligner *al, gbx_mem_align_stats *stats);

/* -------------------------------------------------------------------- kmer
 * Canonical k-mer counting of long reads: Flye's KmerCounter::count as the kmer-cnt benchmark times it
 * (R/benchmarks/kmer-cnt/kmer_cnt.cpp:224-237, vertex_index.cpp:513-612).
 *   R/kmer.h:185-197             IterKmers: a read of len bases gives the k-mers at positions 0 .. len - k - 1, that is
 *                                max(0, len - k) of them (the window ending at the last base is not counted)
 *   R/kmer.h:39-63               code = 2 bits per base, A C G T = 0 1 2 3, first base most significant; the canonical form
 *                                is min(code, revcomp(code)), the complement of base b being 3 - b
 *   R/vertex_index.cpp:537       each read once, on its forward strand
 *   R/vertex_index.cpp:540-577   the flat 4-bit counter saturates at 15 and spills into the cuckoo map, so a k-mer's count
 *                                is 15 + its map value: "Total k-mers" = n_distinct, "Hash size" = n_ge16 below
 *   R/vertex_index.cpp:518-521   k > 17 is refused
 * The reads' filter (length > max(--min-read, --min-ovlp), R/sequence_container.cpp:102) and the treatment of non-ACGT
 * characters (on LP64 the reference's DnaSequence packing turns such a base and the rest of its 32-base chunk into T; see
 * DESIGN 3.7) belong to the parser, not to these entries: every read given is counted.
 * Reads are base codes 0..3, one per byte, read r = enc[read_off[r] ..+ read_len[r]), as gbx_fmi_smem_host takes them.  The
 * CONTRACT is codes 0..3: larger values are not checked (the kernels use their low two bits).
 * Results (exact, independent of the scheduling):
 *   st->n_positions  sum of max(0, len - k); at or above 2^32 the host entry returns GBX_ERR_UNSUPPORTED (32-bit counters)
 *                    and the device entry counts nothing and sets the four fields below to -1
 *   st->n_distinct   distinct canonical k-mers;  st->n_ge16 those counted at least 16 times;  st->max_count the largest count
 *   hist[n_hist]     hist[f] = canonical k-mers counted f times for 1 <= f < n_hist - 1, hist[n_hist - 1] = those counted at
 *                    least n_hist - 1 times, hist[0] = 0 (Flye's _kmerDistribution, vertex_index.cpp:586-602);
 *                    n_hist = 0: no histogram (hist may be NULL), else 2..GBX_KMER_MAX_HIST
 *   selection        the canonical k-mers with min_freq <= count <= max_freq (max_freq 0: no upper bound; min_freq 0:
 *                    nothing is selected) as (sel_kmer, sel_count) pairs in ascending canonical code; st->n_selected is
 *                    their number and may exceed sel_cap, when only the first sel_cap were written
 * The count is a direct-address table of 32-bit counters over the 4^k codes, in slices of 2^30 counters: one pass over
 * the reads for k <= 15, 4 for k = 16, 16 for k = 17; the workspace is about 4^min(k, 15) x 4 bytes (4 GB from k = 15). */
#define GBX_KMER_MAX_K    17
#define GBX_KMER_MAX_HIST 4096
typedef struct gbx_kmer_params {
    int32_t k;           /* 1..17 (the reference's flat-counter limit) */
    int32_t n_hist;      /* hist[f] for 1 <= f < n_hist-1; hist[n_hist-1] = count >= n_hist-1; hist[0] = 0 */
    uint32_t min_freq;   /* selection: canonical k-mers with min_freq <= count <= max_freq ... */
    uint32_t max_freq;   /* ... 0 = no upper bound; min_freq 0 = select nothing */
} gbx_kmer_params;
typedef struct gbx_kmer_stats {
    int64_t n_positions; /* k-mers counted: sum of max(0, len - k) */
    int64_t n_distinct;  /* the reference's "Total k-mers" */
    int64_t n_ge16;      /* the reference's "Hash size" */
    int64_t max_count;
    int64_t n_selected;  /* may exceed sel_cap: then the output did not fit */
} gbx_kmer_stats;

/* Host-buffer entry.  Every read is checked (inside enc_bytes) and the positions counted before the device is touched.
 * A selection larger than sel_cap gives GBX_ERR_ARG with the needed count in st->n_selected and in gbx_last_error(); st and
 * hist are filled then too.  Safe under concurrent host threads; calls are serialised (a call's table is up to 4 GB of
 * device memory, kept between calls like the other host entries' buffers, gbx_host_release frees it).  It runs on the
 * calling thread's current device also when gbx_host_set_devices(n > 1) is in force: the key-space slices would spread
 * over devices naturally, but that is not built. */
int gbx_kmer_count_host(const gbx_kmer_params *p, int64_t n_reads, const uint8_t *enc, int64_t enc_bytes,
                        const int64_t *read_off, const int32_t *read_len, gbx_kmer_stats *st, int64_t *hist,
                        uint64_t *sel_kmer, uint32_t *sel_count, int64_t sel_cap);
/* Device path: every pointer is device memory, the work is queued on `stream` and nothing is synchronised.  *d_stats,
 * d_hist and the selection are written on the device (nothing past sel_cap).  The workspace (gbx_kmer_workspace_bytes)
 * holds the units of the reads and the counter table of one slice. */
size_t gbx_kmer_workspace_bytes(int32_t k, int64_t n_reads, int32_t n_hist);
int gbx_kmer_count_device(const gbx_kmer_params *p, int64_t n_reads, const uint8_t *d_enc, const int64_t *d_read_off,
                          const int32_t *d_read_len, gbx_kmer_stats *d_stats, int64_t *d_hist, uint64_t *d_sel_kmer,
                          uint32_t *d_sel_count, int64_t sel_cap, void *d_work, size_t work_bytes, void *stream);

/* -------------------------------------------------------------- kmer index
 * Flye's minimizer index of long reads: VertexIndex::buildIndexMinimizers(1, window) as the kmer-cnt benchmark times it with
 * use_minimizers = 1 (R/benchmarks/kmer-cnt/kmer_cnt.cpp:228-233, vertex_index.cpp:389-497, kmer.h:206-262).  DESIGN 3.7.1.
 * Reads as the count entries take them (codes 0..3 a byte, larger values use their low two bits); k-mers at positions
 * 0 .. len - k - 1, canonical = min(code, revcomp), "reversed" only when revcomp < code; hash = splitmix64 of the canonical
 * code.  Per read the minimizers are the front positions of the reference's monotone deque over windows of `window`
 * positions, ties as it breaks them (the earlier of two equal hashes stays until it expires, then the last of the equal
 * run takes over); window = 1 chooses every position.
 * The index: a canonical k-mer's capacity is its number of chosen positions; mean_frequency = (float)chosen /
 * (float)(distinct + 1) and repetitive_frequency = (uint64)(repeat_rate * mean_frequency), both in fp32 as the reference
 * rounds them; a k-mer with capacity > repetitive_frequency is repetitive and left out.  Every other chosen position is
 * stored as the global position of the canonical strand's copy: read r of L bases starts at G_r = 2 * (the lengths of the
 * reads before it), a forward k-mer at p has G_r + p, a reversed one G_r + L + (L - p - k).
 * Results (exact, independent of the scheduling): kmer[] the kept k-mers in ascending canonical code, k-mer j's positions
 * pos[off[j] .. off[j + 1]) ascending.  The reference's min_coverage is always 1 and no capacity is below 1: left out. */
#define GBX_KMER_INDEX_MAX_K       31   /* the reference's own mask, 1 << 2k, is undefined at 32 */
#define GBX_KMER_INDEX_MAX_WINDOW  64
typedef struct gbx_kmer_index_params {
    int32_t k;           /* 1..31 */
    int32_t window;      /* 1..64 */
    float repeat_rate;   /* Flye's repeat_kmer_rate, 0 .. 2^20 */
    int32_t reserved_;   /* 0 */
} gbx_kmer_index_params;
typedef struct gbx_kmer_index_stats {
    int64_t n_chosen;               /* minimizer positions of all reads */
    int64_t n_distinct;             /* canonical k-mers among them */
    int64_t repetitive_frequency;   /* "Repetitive k-mer frequency" */
    int64_t n_repetitive_kmers;     /* k-mers left out ... */
    int64_t n_repetitive_entries;   /* ... and the sum of their capacities: "Filtered N repetitive k-mers" */
    int64_t n_selected;             /* "Selected k-mers": may exceed kmer_cap, then the output did not fit */
    int64_t n_entries;              /* "K-mer index size": may exceed pos_cap */
    int64_t total_len;              /* sum of the read lengths */
    float mean_frequency;           /* the filter's "Mean k-mer frequency" */
    int32_t reserved_;
} gbx_kmer_index_stats;

/* The selection alone.  Read r's chosen positions are mini_pos[mini_off[r] .. mini_off[r + 1]) ascending, mini_rev[] 1 where
 * the k-mer there is reversed; mini_off has n_reads + 1 entries.  *n_mini = mini_off[n_reads] is the needed count; nothing is
 * written past mini_cap, and the host entry returns GBX_ERR_ARG when it is larger.  Limits, checked on the host before any
 * device work: every read inside enc_bytes; 2 * total_len < 2^40, else GBX_ERR_UNSUPPORTED. */
int gbx_kmer_minimizers_host(const gbx_kmer_index_params *p, int64_t n_reads, const uint8_t *enc, int64_t enc_bytes,
                             const int64_t *read_off, const int32_t *read_len, int64_t *mini_off, int32_t *mini_pos,
                             uint8_t *mini_rev, int64_t mini_cap, int64_t *n_mini);
/* Host-buffer entry of the index.  kmer[kmer_cap], off[kmer_cap + 1], pos[pos_cap]; a result that does not fit gives
 * GBX_ERR_ARG with the needed counts in st->n_selected / st->n_entries and in gbx_last_error(); st is filled then too.  The
 * limits of gbx_kmer_minimizers_host.  Calls are serialised; it runs on the calling thread's current device. */
int gbx_kmer_index_host(const gbx_kmer_index_params *p, int64_t n_reads, const uint8_t *enc, int64_t enc_bytes,
                        const int64_t *read_off, const int32_t *read_len, gbx_kmer_index_stats *st, uint64_t *kmer,
                        int64_t *off, int64_t kmer_cap, uint64_t *pos, int64_t pos_cap);
/* Device path: every pointer is device memory, the work is queued on `stream` and nothing is synchronised.  total_len is the
 * sum of the read lengths (negative lengths count as 0); the device checks it, and with another sum nothing is selected and
 * every count is -1.  The workspace holds two bytes a base, the tiles' counts and, for the index, the sort's buffers: 48
 * bytes a base (any position can be a minimizer).  index = 0 sizes it for gbx_kmer_minimizers_device alone; 0 for arguments
 * outside the limits. */
size_t gbx_kmer_index_workspace_bytes(int32_t k, int64_t n_reads, int64_t total_len, int32_t index);
int gbx_kmer_minimizers_device(const gbx_kmer_index_params *p, int64_t n_reads, const uint8_t *d_enc,
                               const int64_t *d_read_off, const int32_t *d_read_len, int64_t total_len, int64_t *d_mini_off,
                               int32_t *d_mini_pos, uint8_t *d_mini_rev, int64_t mini_cap, int64_t *d_n_mini, void *d_work,
                               size_t work_bytes, void *stream);
int gbx_kmer_index_device(const gbx_kmer_index_params *p, int64_t n_reads, const uint8_t *d_enc, const int64_t *d_read_off,
                          const int32_t *d_read_len, int64_t total_len, gbx_kmer_index_stats *d_stats, uint64_t *d_kmer,
                          int64_t *d_off, int64_t kmer_cap, uint64_t *d_pos, int64_t pos_cap, void *d_work,
                          size_t work_bytes, void *stream);

/* ------------------------------------------------------------------ pileup
 * medaka's pileup feature counts over a region of aligned long reads: calculate_pileup as the pileup benchmark times it
 * (R/benchmarks/pileup/medaka_counts.c:298-478).  Points marked UPSTREAM rest on htslib's pileup engine.
 * Reads are given already filtered (the benchmark's read filter, medaka_bamiter.c: no UNMAP / SECONDARY / SUPPLEMENTARY /
 * QCFAIL / DUP flag, mapq >= 1, on the region's contig), in BAM's own encodings, sorted by pos (non-decreasing, as a
 * coordinate-sorted BAM holds them):
 *   pos[r]                      0-based leftmost reference position (BAM pos)
 *   cigar[cigar_off[r] ..+)     BAM CIGAR words len << 4 | op, op 0..8 = M I D N S H P = X; cigar_off has n_reads + 1 entries
 *   seq_off[r] .. seq_off[r+1]  read r's bases: l_seq = seq_off[r+1] - seq_off[r], qualities qual[seq_off[r] ..+ l_seq)
 *                               (0xFF = missing), nt16 codes packed two a byte, first base in the high nibble, from byte
 *                               seq[seq_boff[r]] (BAM's (l_seq + 1) / 2 bytes)
 *   rev[r]                      1: reverse strand (BAM flag 0x10);  dtype[r]: the index of the read's DT:Z value among the
 *                               caller's dtypes, -1 when it has none (may be NULL when num_dtypes == 1)
 * A read spans [pos, pos + its M D N = X lengths).  Every position p in [start, end) that some read spans has
 * 1 + max_ins columns (major = p, minor = 0 .. max_ins), max_ins the largest positive indel among p's pileup entries
 * (refskip entries included); positions no read spans have none.  pos_col[p - start] is the first column of p,
 * pos_col[end - start] = n_cols.  Entries (UPSTREAM: htslib resolve_cigar2): an M = X position gives a base at its query
 * position, D a deletion, N a refskip; at the last position of an op the next op gives indel: I +len, D after a non-D op
 * -len, P then the sum of the I lengths up to the next op that consumes the reference.
 * Counts: F = 10 * num_dtypes * num_homop uint32 per column, index (dtype * num_homop + stratum) * 10 + b with b in
 * "acgtACGTdD".  A deletion adds 1 to d (reverse) or D (forward) at stratum 0; a base entry with indel i adds, for
 * j = 0 .. max(i, 0), base seq[qpos + j] (IUPAC codes other than A C G T: nothing) to column j of the position at stratum
 * max(0, min(qual[qpos + j], num_homop) - 1) (0 when num_homop == 1); refskip entries add nothing.  The counts are exact
 * and do not depend on the scheduling, the slicing or the number of devices.
 * Not modelled: htslib's cap of 8000 reads per start position, Weibull summation (GBX_ERR_UNSUPPORTED). */
#define GBX_PILEUP_FEATLEN    10
#define GBX_PILEUP_MAX_DTYPES 64
#define GBX_PILEUP_MAX_HOMOP  64
#define GBX_PILEUP_MAX_F      10240   /* 10 * num_dtypes * num_homop */
typedef struct gbx_pileup_params {
    int32_t num_dtypes;      /* 1..64 */
    int32_t num_homop;       /* 1..64 quality strata; num_dtypes * num_homop <= 1024 */
    int64_t start, end;      /* the region [start, end), 0-based, 0 <= start <= end < 2^31 */
    int64_t slice_positions; /* host entries: at most this many positions per device slice; 0 = the default, 2^22 (a test
                                aid: any value >= 1 gives the same results) */
    int32_t weibull;         /* must be 0: Weibull summation is not built */
    int32_t pad_;
} gbx_pileup_params;
typedef struct gbx_pileup_reads {
    int64_t n_reads;
    int64_t seq_bytes;       /* bytes of seq (host entries check every read against it) */
    const int32_t *pos;
    const int64_t *cigar_off;
    const uint32_t *cigar;
    const int64_t *seq_off;
    const int64_t *seq_boff;
    const uint8_t *seq;
    const uint8_t *qual;
    const uint8_t *rev;
    const int8_t *dtype;
} gbx_pileup_reads;
typedef struct gbx_pileup_layout_stats {
    int64_t n_cols;          /* pos_col[end - start] */
    int64_t n_positions;     /* positions with columns */
    int64_t max_ins;
    int64_t max_depth;       /* reads spanning one position, at most */
    int64_t aligned_bases;   /* M = X positions of the reads inside [start, end) */
    int64_t bad_read;        /* num_dtypes > 1: the lowest read without a valid dtype that has a non-refskip entry in the
                                region, else -1 */
} gbx_pileup_layout_stats;

/* Host-buffer entries.  Every read is checked (ops, l_seq against the query length of its CIGAR, offsets inside their
 * arrays, pos sorted and below 2^31) before the device is touched.  The region is cut into slices, spread over the devices
 * of gbx_host_set_devices / GBX_GPUS by their aligned bases.  A slice's device memory is about 40 bytes a position, 8 + 4 F
 * a column and its reads: the layout's slices hold at most slice_positions positions; the count's, cut from pos_col, also at
 * most 64 M counters (256 MB) of columns, unless one position alone has more.
 * layout: pos_col[end - start + 1] and *st; a read without a valid dtype (st->bad_read >= 0) gives GBX_ERR_ARG, with pos_col
 * and *st filled.
 * count: the columns of positions [p0, p1) (start <= p0 <= p1 <= end) of the layout pos_col: c = pos_col[p1 - start] -
 * pos_col[p0 - start] of them, major[c], minor[c] and counts[c * F]; a sub-range bounds the caller's memory. */
int gbx_pileup_layout_host(const gbx_pileup_params *p, const gbx_pileup_reads *reads, int64_t *pos_col,
                           gbx_pileup_layout_stats *st);
int gbx_pileup_count_host(const gbx_pileup_params *p, const gbx_pileup_reads *reads, const int64_t *pos_col, int64_t p0,
                          int64_t p1, int32_t *major, int32_t *minor, uint32_t *counts);
/* Device path: `reads` is a host struct whose pointers are device memory; every other pointer is device memory, the work
 * is queued on `stream` and nothing is synchronised; the whole region is one slice.  count takes the pos_col the layout
 * wrote; entries of a read without a valid dtype are not counted there (the layout's bad_read reports them).  The
 * workspace (gbx_pileup_workspace_bytes) serves both. */
size_t gbx_pileup_workspace_bytes(const gbx_pileup_params *p, int64_t n_reads, int64_t n_cigar);
int gbx_pileup_layout_device(const gbx_pileup_params *p, const gbx_pileup_reads *reads, int64_t *d_pos_col,
                             gbx_pileup_layout_stats *d_stats, void *d_work, size_t work_bytes, void *stream);
int gbx_pileup_count_device(const gbx_pileup_params *p, const gbx_pileup_reads *reads, const int64_t *d_pos_col, int64_t p0,
                            int64_t p1, int32_t *d_major, int32_t *d_minor, uint32_t *d_counts, void *d_work,
                            size_t work_bytes, void *stream);

/* --------------------------------------------------------------------- dbg
 * Platypus's de Bruijn graph assembly of a BAM region as the dbg benchmark times it: one graph per assembly window, built
 * and destroyed (R/benchmarks/dbg/debruijn.cpp:1565-1589; cycle detection there is commented out).  Points marked UPSTREAM
 * rest on htslib (the region iterator, bam_endpos, faidx) and are not confirmed by anything in the tree.
 * Reads (gbx_dbg_reads), in the order the region iterator returns them (file order, no filter):
 *   seq[seq_off[r] ..+ l_seq]    ASCII bases (BAM nt16 through "=ACMGRSVTWYHKDBN"), qual the raw qualities, flag the BAM flag
 *   pos[r]                       BAM pos minus the length of a leading S op, as uint32 (wraps below 0)
 *   end[r]                       bam_endpos (UPSTREAM: pos + reference length, or pos + 1 when unmapped or of length 0)
 * Windows (gbx_dbg_windows): for a = beg, beg + shift, ... while a < end, shift = max(100, min(1000, region_size / 2)):
 *   assem [a, min(a + region_size, end)), ref [max(0, a - region_size), assem_end + region_size) clamped to the contig by the
 *   caller's FASTA fetch (UPSTREAM: faidx), bytes as stored.  Its reads: lo = bisect_left(pos, max(1, a - longest)) then lo
 *   advances while end[lo] <= a, hi = bisect_left(pos, assem_end), reads [lo, min(hi, n)), every comparison unsigned (uint32),
 *   longest = max over reads of (int32)(end - pos) and 0; lo > hi is the reference's fatal error.
 * The graph of a window (k, min_qual): edge occurrences, in this order,
 *   the reference's i = 0 .. ref_len - k - 2: k-mer i -> k-mer i + 1, weight 1, colour REF (1), positions ref_pos + i (+ 1);
 *   then every read of the window without flag 0x200, i = 0 .. l_seq - k - 2: its k + 1 bases [i, i + k], skipped when one
 *   of them is 'N' or their minimum quality is below min_qual; else weight = that minimum, colour READ (2), position -1.
 * Each occurrence touches its start node, then its end node (identity: the k bytes, case-sensitive); a new node takes the
 * occurrence's colour, position and weight, an existing one gets colours |= and weight +=.  The edge: the start node's edge
 * to that end node grows by the weight, or is appended when the node has fewer than 4, or is dropped.  So a node's weight
 * is the sum over its touches, its position comes from its first touch, the nodes are in first-touch order, and an edge
 * is kept iff it is among the first 4 distinct successors of its start node by first appearance (its weight: all of its
 * occurrences).  The graph is exact and does not depend on scheduling or device count.
 * Digest: FNV-1a 64 (offset basis 0xcbf29ce484222325, prime 0x100000001b3) over every node in first-touch order:
 *   its k bytes, colours (1 byte), position (int32 LE), weight (int64 LE), n_edges (1 byte), then for each kept edge in
 *   order of first appearance the end node's index in first-touch order (int32 LE) and the edge weight (int64 LE). */
#define GBX_DBG_MIN_K    3
#define GBX_DBG_MAX_K    64
#define GBX_DBG_REF      1
#define GBX_DBG_READ     2
typedef struct gbx_dbg_params {
    int32_t k;               /* 3..64; 15 in the benchmark */
    int32_t min_qual;        /* 0..255; 20 */
    int32_t region_size;     /* >= 1; 1500 */
    int32_t pad_;
} gbx_dbg_params;
void gbx_dbg_default_params(gbx_dbg_params *p);
typedef struct gbx_dbg_reads {
    int64_t n_reads;
    int64_t seq_bytes;       /* bytes of seq and qual */
    const int64_t *seq_off;  /* n_reads + 1, non-decreasing, seq_off[n_reads] <= seq_bytes */
    const uint8_t *seq;
    const uint8_t *qual;
    const uint16_t *flag;
    const uint32_t *pos;     /* gbx_dbg_windows only (may be NULL elsewhere) */
    const uint32_t *end;     /* gbx_dbg_windows only */
} gbx_dbg_reads;
typedef struct gbx_dbg_wins {
    int64_t n_win;
    int64_t ref_bytes;       /* bytes of ref */
    const int64_t *ref_off;  /* n_win + 1: window w's reference is ref[ref_off[w] .. ref_off[w + 1]) */
    const uint8_t *ref;
    const int64_t *ref_pos;  /* the reference position of its first byte (refStart) */
    const int64_t *read_lo;  /* its reads [read_lo, read_hi) */
    const int64_t *read_hi;
} gbx_dbg_wins;
typedef struct gbx_dbg_stats {
    int64_t n_nodes;
    int64_t n_edges;         /* kept */
    int64_t n_dropped;       /* distinct successors past the 4th */
    int64_t n_occ;           /* edge occurrences inserted */
    int64_t weight_sum;      /* their weights */
    int64_t n_ref, n_read, n_both;   /* nodes by colours: REF only, READ only, both */
    uint64_t digest;
} gbx_dbg_stats;
typedef struct gbx_dbg_node {
    int64_t weight;
    int64_t src;             /* where its first touch read it: >= 0 a byte offset in ref, < 0: -1 - a byte offset in seq */
    int64_t first_edge;      /* its edges are edges[first_edge ..+ n_edges] (indices into the call's edge array) */
    int32_t position;
    uint8_t colours;
    uint8_t n_edges;
    uint8_t pad_[2];
} gbx_dbg_node;
typedef struct gbx_dbg_edge {
    int64_t weight;
    int32_t end;             /* the end node's index in its window's first-touch order */
    int32_t pad_;
} gbx_dbg_edge;

/* Host only (no device): the windows of [beg, end) (0 <= beg, end < 2^31) and their read ranges.  n_win receives their
 * number; with cap >= it, assem_start / assem_end / ref_start / ref_end / read_lo / read_hi[0 .. n_win) are filled (any
 * may be NULL).  lo > hi: GBX_ERR_ARG, *n_win = the failing window + 1 and its raw lo / hi written when cap allows. */
int gbx_dbg_windows(const gbx_dbg_params *p, const gbx_dbg_reads *reads, int64_t beg, int64_t end, int64_t cap, int64_t *n_win,
                    int64_t *assem_start, int64_t *assem_end, int64_t *ref_start, int64_t *ref_end, int64_t *read_lo, int64_t *read_hi);
/* The benchmark step: every window's graph, stats[n_win].  Reads and windows are checked before the device is touched;
 * windows are spread over the devices of gbx_host_set_devices / GBX_GPUS by their occurrences. */
int gbx_dbg_build_host(const gbx_dbg_params *p, const gbx_dbg_reads *reads, const gbx_dbg_wins *wins, gbx_dbg_stats *stats);
/* The graphs of windows [w0, w1): node_off / edge_off[w1 - w0 + 1] place window w0 + j's nodes at nodes[node_off[j] ..)
 * and its kept edges at edges[edge_off[j] ..) (prefix sums of the stats' n_nodes and n_edges; the range bounds memory). */
int gbx_dbg_graph_host(const gbx_dbg_params *p, const gbx_dbg_reads *reads, const gbx_dbg_wins *wins, int64_t w0, int64_t w1,
                       const int64_t *node_off, const int64_t *edge_off, gbx_dbg_node *nodes, gbx_dbg_edge *edges);
/* Device path: `reads` and `wins` are host structs whose pointers are device memory, as are every other pointer; the call
 * reads the offsets and ranges back once to plan its passes (it synchronises `stream` there), then queues the rest.
 * max_window_occ: the most occurrence slots of one window, max over w of max(0, ref_len - k - 1) + sum over its reads of
 * max(0, l_seq - k - 1); the workspace holds at least that window. */
size_t gbx_dbg_workspace_bytes(const gbx_dbg_params *p, int64_t n_win, int64_t n_reads, int64_t max_window_occ);
int gbx_dbg_build_device(const gbx_dbg_params *p, const gbx_dbg_reads *reads, const gbx_dbg_wins *wins, gbx_dbg_stats *d_stats,
                         void *d_work, size_t work_bytes, void *stream);
int gbx_dbg_graph_device(const gbx_dbg_params *p, const gbx_dbg_reads *reads, const gbx_dbg_wins *wins, int64_t w0, int64_t w1,
                         const int64_t *d_node_off, const int64_t *d_edge_off, gbx_dbg_node *d_nodes, gbx_dbg_edge *d_edges,
                         void *d_work, size_t work_bytes, void *stream);

/* ------------------------------------------------------------- dbg_asm: cycle check, k-mer retry, variant paths
 * What Platypus's assembler does with each window's graph behind the build: the cycle check
 * (R/benchmarks/dbg/debruijn.cpp:923-998, dfsVisit / detectCyclesInGraph_Recursive), the rebuild at a larger k while the
 * graph is cyclic (1408-1428, commented out in the benchmark) and the variant paths (1094-1239, checkPathForCycles,
 * getVariantPathsThroughGraphFromNode, createSequenceFromPath).  All of it reads the graph of the dbg section (nodes in
 * first-touch order, at most 4 kept edges per node in order of first appearance) and changes nothing there.  Pinned by
 * the restatement tests/dbg_asm_ref.py; the start rule is UPSTREAM (Platypus's findBubbles, not in the reference tree).
 * Weights are whole numbers, every comparison is on integers.
 * Cycle check: the window is cyclic iff the directed graph of its counted edges has a cycle (a self-loop is one).  An
 *   edge is not counted when its end node's colours are READ only and its weight is below min_weight; an edge into a REF
 *   or REF|READ node counts whatever its weight.  This is detectCyclesInGraph_Recursive's return value; it does not depend
 *   on the visiting order.
 * Retry: a window starts at the dbg params' k; while its graph is cyclic and k <= k_last it is rebuilt at k + k_step
 *   (15, 20, .., 55 by default; a window still cyclic at 55 stays at 55 with cyclic = 1).  Every k reached must lie in
 *   GBX_DBG_MIN_K..GBX_DBG_MAX_K (checked up front for the largest k any window can reach).  A window's graph at a k is
 *   exactly gbx_dbg_build_*'s at that k: a reference shorter than k + 2 contributes nothing, and without reads the graph
 *   is empty and acyclic.
 * Variant paths, on the final graph of every window (cyclic ones too):
 *   starts (UPSTREAM)   nodes in first-touch order, then their edges in edge order: a node of colours REF|READ with a kept
 *                       edge of weight >= min_weight whose end node is READ only.  The start path is the two nodes, its
 *                       weight that edge's weight.
 *   search              a LIFO stack of paths holding the start path, and a list of finished paths.  While the stack is
 *                       not empty, pop P, then in this order: count a step, more than max_steps: status STEPS, no paths;
 *                       more than max_pending paths left on the stack or more than max_finished finished: status GAVE_UP,
 *                       no paths; P's last node occurs earlier in P: drop P; its last node is REF|READ: P is finished;
 *                       REF only: drop P; else for each kept edge of the last node in edge order, when its weight is
 *                       >= min_weight or its end node has REF among its colours, push P + that end node, weight P's plus
 *                       the edge's.  max_steps is this library's own bound (none in the reference).
 *   a path              its node indices (first-touch order of its window), its weight, the positions of its first and
 *                       last node, and its sequence: one byte per node, the first byte of the node's k-mer.
 * Output (gbx_dbg_asm_out), against the caller's capacities: per window a gbx_dbg_asm_win and the final graph's
 * gbx_dbg_stats; starts[], paths[], path_nodes[] / path_seq[].  A window's starts are starts[first_start ..+ n_starts] in
 * the order above; a start's paths are paths[first_path ..+ n_paths] in finishing order; a path's nodes are
 * path_nodes[first_node ..+ n_nodes] and its bytes path_seq at the same place.  The windows' blocks of starts lie in the
 * order the windows became final: by round, then by window index (so the layout is a function of the input alone).
 * totals[0..2] receive the starts, paths and path nodes of the whole call; where one exceeds its capacity the arrays hold
 * what fitted (every index below the capacity is as it would be with room), totals says what to allocate, and the entry
 * returns GBX_ERR_UNSUPPORTED with the sizes in the error text.  k, n_builds, cyclic, stats and n_starts are complete
 * either way; a start that did not fit is not searched, so with cap_starts short the paths' totals and the windows' path
 * counts cover the starts that fitted (n_starts <= n_edges of the final graphs bounds the starts beforehand). */
#define GBX_DBG_ASM_OK        0
#define GBX_DBG_ASM_GAVE_UP   1
#define GBX_DBG_ASM_STEPS     2
#define GBX_DBG_ASM_MAX_PENDING 59    /* the stack of one search holds max_pending + 4 paths at most: 63 */
typedef struct gbx_dbg_asm_params {
    int32_t min_weight;      /* >= 0; 40 (the reference's minReads * minQual) */
    int32_t k_step;          /* >= 1; 5 */
    int32_t k_last;          /* rebuild while k <= k_last; 50.  Below the dbg params' k: no retry */
    int32_t max_pending;     /* 0..GBX_DBG_ASM_MAX_PENDING; 20 */
    int32_t max_finished;    /* >= 0; 20 */
    int32_t pad_;
    int64_t max_steps;       /* >= 0; 2^20 */
} gbx_dbg_asm_params;
void gbx_dbg_asm_default_params(gbx_dbg_asm_params *p);
typedef struct gbx_dbg_asm_win {
    int32_t k;               /* of the final graph */
    int32_t n_builds;
    int32_t cyclic;          /* of the final graph */
    int32_t pad_;
    int64_t first_start, n_starts;
    int64_t n_paths, n_path_nodes;    /* over its starts of status OK */
    int64_t n_gave_up, n_steps;       /* starts of status GAVE_UP / STEPS */
} gbx_dbg_asm_win;
typedef struct gbx_dbg_asm_start {
    int64_t first_path, n_paths;      /* n_paths = 0 unless status is OK */
    int64_t first_node, n_nodes;      /* its paths' nodes are contiguous: path_nodes[first_node ..+ n_nodes] */
    int32_t win, node, edge, status;  /* edge: the number of the start edge among the node's kept edges */
} gbx_dbg_asm_start;
typedef struct gbx_dbg_asm_path {
    int64_t weight;
    int64_t first_node;
    int32_t n_nodes;
    int32_t pos_first, pos_last;      /* gbx_dbg_node.position of the first and last node (-1: a READ-only node) */
    int32_t pad_;
} gbx_dbg_asm_path;
typedef struct gbx_dbg_asm_out {
    gbx_dbg_stats *stats;             /* n_win */
    gbx_dbg_asm_win *wins;            /* n_win */
    gbx_dbg_asm_start *starts;
    gbx_dbg_asm_path *paths;
    int32_t *path_nodes;
    uint8_t *path_seq;
    int64_t cap_starts, cap_paths, cap_path_nodes;
    int64_t *totals;                  /* 3 */
} gbx_dbg_asm_out;
/* Reads and windows as gbx_dbg_build_host; one device (no spreading over devices). */
int gbx_dbg_assemble_host(const gbx_dbg_params *p, const gbx_dbg_asm_params *ap, const gbx_dbg_reads *reads, const gbx_dbg_wins *wins,
                          const gbx_dbg_asm_out *out);
/* Device path, the contract of gbx_dbg_build_device: every pointer inside reads, wins and out is device memory.  The call
 * reads the offsets and ranges back once, and after every round the windows' cyclic flags, to plan the next round (it
 * synchronises `stream` there); totals are read back at the end for the return value.  The graphs are taken in ranges of
 * windows that fit the workspace (tables, nodes at 2 * occ and edges at occ per window), at least one window.
 * max_window_occ as in gbx_dbg_workspace_bytes, at the dbg params' k (larger k have fewer slots). */
size_t gbx_dbg_assemble_workspace_bytes(const gbx_dbg_params *p, int64_t n_win, int64_t n_reads, int64_t max_window_occ);
int gbx_dbg_assemble_device(const gbx_dbg_params *p, const gbx_dbg_asm_params *ap, const gbx_dbg_reads *reads, const gbx_dbg_wins *wins,
                            const gbx_dbg_asm_out *out, void *d_work, size_t work_bytes, void *stream);

/* ------------------------------------------------------------------- mm: minimizer seeding in front of chain
 * minimap2's seeding stage: the minimizer sketch (mm_sketch), the minimizer index (mm_idx_*) and seed collection with the
 * occurrence filter (collect_matches + collect_seed_hits): what fmi + fmi_sal are for bsw, this is for chain.  UNPINNED by a
 * compiled reference (minimap2's source is not part of the reference tree): the rules are restated in full in DESIGN 3.18 and
 * tests/mm_ref.py, and pinned by that restatement.
 * Sequences are text, one byte per base: A C G T in either case are codes 0..3, every other byte is ambiguous.  Sequence s =
 * seq[seq_off[s] .. seq_off[s + 1]); seq_off[0] = 0, never decreasing.
 *   sketch   the (x, y) pairs of minimap2's sequential machine, bit for bit and in its order: x = hash64(k-mer) << 8 | span,
 *            y = rid << 32 | last base << 1 | strand.  A sequence is taken in pieces of GBX_MM_SKETCH_CHUNK bases, each
 *            warm-started w + k steps ahead (exact for odd k; for even k a sequence is one piece, one lane).
 *   index    the minimizers of every reference sequence (rid = its ordinal) grouped by x >> 8: sorted distinct keys, a CSR of
 *            their values y in ascending order (minimap2's order inside a key comes from an unstable sort), and mid_occ
 *   seeding  per read (rid 0): every minimizer whose key occurs fewer than mid_occ times gives one anchor per occurrence,
 *            the others feed rep_len; a read's anchors ascending by x, ties by the whole of y (minimap2 sorts by x alone,
 *            unstably); the output is a chain batch: off, ax, ay and one gbx_chain_call per read.
 * Not modelled: multi-segment reads, index batches and .mmi files, the self / dual filters, re-seeding. */
#define GBX_MM_SKETCH_CHUNK 256
#define GBX_MM_SEED_TANDEM  (1ull << 42)   /* MM_SEED_TANDEM in ay */
#define GBX_MM_MAX_READS    (1 << 21)      /* reads of one seeding call (the sort key holds the read in 21 bits) */
typedef struct gbx_mm_params {
    int32_t k;             /* 15; 1..28 */
    int32_t w;             /* 10; 1..255 */
    int32_t is_hpc;        /* 0; homopolymer-compressed k-mers */
    int32_t mid_occ;       /* 0: from mid_occ_frac; > 0: the threshold itself */
    float   mid_occ_frac;  /* 2e-4; <= 0: INT32_MAX; below 1 */
    int32_t max_gap;       /* 5000: max_dist_x = max_dist_y of the calls */
    int32_t bw;            /* 500 */
} gbx_mm_params;
typedef struct gbx_mm_index_info {
    int64_t n_keys, n_vals;    /* distinct keys, minimizers */
    int32_t mid_occ;
    int32_t k, w, is_hpc;      /* what it was built with */
} gbx_mm_index_info;

void gbx_mm_default_params(gbx_mm_params *p);
/* GBX_ERR_ARG naming the field: k outside 1..28, w outside 1..255, a negative mid_occ, max_gap or bw, a mid_occ_frac that is not
 * a number or is 1 or more.  Needs no device. */
int gbx_mm_check_params(const gbx_mm_params *p);

/* Sketch of n_seqs sequences (total_len = seq_off[n_seqs] bytes).  rid_ordinal != 0: sequence s has rid s, else every rid is 0.
 * Sequence s owns minimizers [mini_off[s], mini_off[s + 1]); *n_mini = their number, which may exceed mini_cap: then only the
 * first mini_cap are written and the offsets stay true.  The device entry does no host synchronisation. */
size_t gbx_mm_sketch_workspace_bytes(const gbx_mm_params *p, int64_t n_seqs, int64_t total_len);
int gbx_mm_sketch_device(const gbx_mm_params *p, int64_t n_seqs, const uint8_t *d_seq, const int64_t *d_seq_off, int64_t total_len,
                         int32_t rid_ordinal, uint64_t *d_mini_x, uint64_t *d_mini_y, int64_t mini_cap, int64_t *d_mini_off,
                         int64_t *d_n_mini, void *d_work, size_t work_bytes, void *stream);
/* Checked before the device is touched, GBX_ERR_ARG naming the lowest offender: null pointers, seq_off[0] != 0, offsets that
 * decrease; GBX_ERR_UNSUPPORTED: a sequence of 2^31 bases or more, 2^31 sequences or more.  More minimizers than mini_cap:
 * GBX_ERR_ARG with the needed count in *n_mini and gbx_last_error() (mini_off is written; call with 0 / NULL to size). */
int gbx_mm_sketch_host(const gbx_mm_params *p, int64_t n_seqs, const uint8_t *seq, const int64_t *seq_off, int32_t rid_ordinal,
                       uint64_t *mini_x, uint64_t *mini_y, int64_t mini_cap, int64_t *mini_off, int64_t *n_mini);

/* The index on the device: one allocation of gbx_mm_index_bytes(mini_cap) bytes for up to mini_cap minimizers (total_len is
 * always enough).  gbx_mm_index_build_device queues the whole build on `stream` without synchronising; gbx_mm_index_stats
 * synchronises it and reads the counts: GBX_ERR_ARG with the need in gbx_last_error() when the reference has more than mini_cap
 * minimizers (such an index must not be used). */
size_t gbx_mm_index_bytes(int64_t mini_cap);
size_t gbx_mm_index_workspace_bytes(const gbx_mm_params *p, int64_t n_seqs, int64_t total_len, int64_t mini_cap);
int gbx_mm_index_build_device(const gbx_mm_params *p, int64_t n_seqs, const uint8_t *d_seq, const int64_t *d_seq_off, int64_t total_len,
                              void *d_index, int64_t mini_cap, void *d_work, size_t work_bytes, void *stream);
int gbx_mm_index_stats(const void *d_index, int64_t mini_cap, gbx_mm_index_info *st, void *stream);
/* Host buffers in and out: keys[key_cap], key_off[key_cap + 1] (key j owns vals[key_off[j] .. key_off[j + 1])), vals[val_cap].
 * The checks of gbx_mm_sketch_host; counts above the capacities: GBX_ERR_ARG with the need in *st and gbx_last_error() (call
 * with 0 / NULL to size). */
int gbx_mm_index_build_host(const gbx_mm_params *p, int64_t n_seqs, const uint8_t *seq, const int64_t *seq_off,
                            uint64_t *keys, int64_t *key_off, int64_t key_cap, uint64_t *vals, int64_t val_cap, gbx_mm_index_info *st);

/* Seeding of n_reads reads (at most GBX_MM_MAX_READS, total_len bytes) against an index built with the same k, w and is_hpc;
 * the index's mid_occ applies.  ref_n_seqs / ref_max_len: the reference's sequence count and longest sequence (they bound the
 * digits the anchor sort visits; larger values are safe).  Output: the chain batch off[n_reads + 1], ax, ay, hdr[n_reads]
 * (avg_qspan = (float)sum of the anchors' spans / their number, 0 without anchors; max_dist_x = max_dist_y = max_gap; bw;
 * n_segs = 1), rep_len[n_reads], n_mini[n_reads], the reads' minimizers (mini_off, mini_x, mini_y) and counts[2] = minimizers,
 * anchors.  A count above its capacity reports the need, nothing is written past a capacity, off and mini_off stay true (with
 * more minimizers than mini_cap the anchors are not made: counts[1] = -1).  The device entry does no host synchronisation. */
size_t gbx_mm_seed_workspace_bytes(const gbx_mm_params *p, int64_t n_reads, int64_t total_len, int64_t mini_cap, int64_t anchor_cap);
int gbx_mm_seed_device(const gbx_mm_params *p, const void *d_index, int64_t index_mini_cap, int64_t ref_n_seqs, int64_t ref_max_len,
                       int64_t n_reads, const uint8_t *d_seq, const int64_t *d_seq_off, int64_t total_len,
                       uint64_t *d_mini_x, uint64_t *d_mini_y, int64_t mini_cap, int64_t *d_mini_off,
                       uint64_t *d_ax, uint64_t *d_ay, int64_t anchor_cap, int64_t *d_off, gbx_chain_call *d_hdr,
                       int32_t *d_rep_len, int32_t *d_n_mini, int64_t *d_counts, void *d_work, size_t work_bytes, void *stream);
/* Host buffers in and out; the index as gbx_mm_index_build_host left it (n_keys keys, mid_occ the threshold to apply).  The
 * checks of gbx_mm_sketch_host on the reads, and on the index: key_off from 0, never decreasing.  mini_x / mini_y / mini_off may
 * be NULL (mini_cap 0).  Counts above the capacities: GBX_ERR_ARG with the needed counts in counts[2] and gbx_last_error() (off,
 * hdr, rep_len and n_mini are written). */
int gbx_mm_seed_host(const gbx_mm_params *p, const uint64_t *keys, const int64_t *key_off, int64_t n_keys, const uint64_t *vals,
                     int32_t mid_occ, int64_t ref_n_seqs, int64_t ref_max_len,
                     int64_t n_reads, const uint8_t *seq, const int64_t *seq_off,
                     uint64_t *mini_x, uint64_t *mini_y, int64_t mini_cap, int64_t *mini_off,
                     uint64_t *ax, uint64_t *ay, int64_t anchor_cap, int64_t *off, gbx_chain_call *hdr,
                     int32_t *rep_len, int32_t *n_mini, int64_t *counts);

/* ------------------------------------------------------------------- mm map: from chain scores to PAF records
 * minimap2 behind the chain DP, as `minimap2 -x map-ont` runs it without -c: the chain ends and the backtrack (second half of
 * mm_chain_dp), mm_gen_regs, mm_set_parent, mm_select_sub, mm_set_mapq and the PAF line.  UNPINNED by a compiled reference, as
 * the seeding stage is: the rules are restated in DESIGN 3.19 and tests/mm_map_ref.py and pinned by that restatement; where
 * minimap2 leaves an order to an unstable sort the rule fixes it.
 * Input: the chain batch of gbx_mm_seed_* (off, ax, ay), chain's score, parent and peak over it (parent local to the call, -1:
 * none; chain leaves parent[i] < i, any other value counts as none), and per read its length, rep_len and a 32-bit hash.
 * Not modelled: mm_join_long, mm_squeeze_a, re-chaining with max_occ, mm_filter_regs, mm_split_reg, inversions, dv:f,
 * mm_set_sam_pri, multi-segment reads, CIGAR. */
typedef struct gbx_mm_map_params {
    int32_t min_cnt;           /* 3; >= 1 */
    int32_t min_chain_score;   /* 40; >= 0 */
    float   mask_level;        /* 0.5 */
    float   pri_ratio;         /* 0.8; <= 0: no selection */
    int32_t best_n;            /* 5; >= 0 */
    int32_t min_diff;          /* 30 = 2k */
} gbx_mm_map_params;
/* One mapping: 72 bytes, 18 words of 4. */
typedef struct gbx_mm_reg {
    int32_t id, parent;        /* within the read; parent == id: a primary */
    int32_t score, subsc;
    int32_t cnt, as;           /* its anchors: cnt from `as` of the read's chained anchors */
    int32_t rid, rev;
    int32_t rs, re, qs, qe;
    int32_t mlen, blen;
    int32_t n_sub, mapq;
    uint32_t hash;
    int32_t read;
} gbx_mm_reg;

void gbx_mm_map_default_params(gbx_mm_map_params *p);
/* GBX_ERR_ARG naming the field: min_cnt < 1, min_chain_score < 0, best_n < 0, a mask_level or pri_ratio that is not a number. */
int gbx_mm_map_check_params(const gbx_mm_map_params *p);

/* Chains and regions of n_reads reads whose anchors fill [0, anchor_cap) at most (anchor_cap >= off[n_reads]).  Output:
 *   chain_off[n_reads + 1], u[chain_cap]   read r's chains [chain_off[r], chain_off[r + 1]), u = score << 32 | anchors, ascending
 *                                          by the x of their first anchor
 *   cax, cay [anchor_cap], n_chained[n_reads]   read r's chained anchors at off[r], n_chained[r] of them, chain after chain
 *   reg_off[n_reads + 1], regs[reg_cap]    read r's regions, in order
 *   counts[2]                              chains, regions
 * A count above its capacity reports the need, nothing is written past a capacity and chain_off stays true; with more chains
 * than chain_cap the regions are not made (counts[1] = -1, reg_off all 0).  The device entry does no host synchronisation. */
size_t gbx_mm_map_workspace_bytes(int64_t n_reads, int64_t anchor_cap, int64_t chain_cap);
int gbx_mm_map_device(const gbx_mm_map_params *p, int64_t n_reads, const int64_t *d_off, const uint64_t *d_ax, const uint64_t *d_ay,
                      int64_t anchor_cap, const int32_t *d_score, const int32_t *d_parent, const int32_t *d_peak,
                      const int64_t *d_seq_off, const int32_t *d_rep_len, const uint32_t *d_hash,
                      int64_t *d_chain_off, uint64_t *d_u, int64_t chain_cap, uint64_t *d_cax, uint64_t *d_cay, int32_t *d_n_chained,
                      int64_t *d_reg_off, gbx_mm_reg *d_regs, int64_t reg_cap, int64_t *d_counts, void *d_work, size_t work_bytes, void *stream);
/* Host buffers in and out; seq_off[n_reads + 1]: the reads' lengths as offsets.  Checked before the device is touched,
 * GBX_ERR_ARG naming the lowest offender: null pointers, off[0] or seq_off[0] != 0, offsets that decrease, negative
 * capacities, a parent outside -1 .. i - 1; GBX_ERR_UNSUPPORTED: more than GBX_MM_MAX_READS reads, a read of 2^31 anchors or
 * bases.  Counts above the capacities: GBX_ERR_ARG with the needed counts in counts[2] and gbx_last_error() (chain_off is
 * written; call with 0 / NULL to size). */
int gbx_mm_map_host(const gbx_mm_map_params *p, int64_t n_reads, const int64_t *off, const uint64_t *ax, const uint64_t *ay,
                    const int32_t *score, const int32_t *parent, const int32_t *peak,
                    const int64_t *seq_off, const int32_t *rep_len, const uint32_t *hash,
                    int64_t *chain_off, uint64_t *u, int64_t chain_cap, uint64_t *cax, uint64_t *cay, int32_t *n_chained,
                    int64_t *reg_off, gbx_mm_reg *regs, int64_t reg_cap, int64_t *counts);

/* PAF text of the regions: one line a region, read after read (a read's lines are lines[line_off[r] .. line_off[r + 1])):
 * qname qlen qs qe +/- tname tlen rs re mlen blen mapq tp:A:P|S cm:i: s1:i: s2:i: (primaries) rl:i:.  Names are byte arenas
 * with offsets; a region whose rid is outside 0 .. n_targets - 1 prints `*` and length 0.  *n_text = the bytes needed, which
 * may exceed text_cap: then nothing is written past it and line_off stays true.  d_n_regs: the region count on the device
 * (counts + 1 of gbx_mm_map_device); regions at and past reg_cap do not exist.  No host synchronisation. */
size_t gbx_mm_paf_workspace_bytes(int64_t n_reads, int64_t reg_cap);
int gbx_mm_paf_device(int64_t n_reads, const gbx_mm_reg *d_regs, const int64_t *d_reg_off, const int64_t *d_n_regs, int64_t reg_cap,
                      const uint8_t *d_qnames, const int64_t *d_qname_off, const int64_t *d_seq_off, const int32_t *d_rep_len,
                      int64_t n_targets, const uint8_t *d_tnames, const int64_t *d_tname_off, const int64_t *d_tseq_off,
                      uint8_t *d_lines, int64_t text_cap, int64_t *d_line_off, int64_t *d_n_text, void *d_work, size_t work_bytes, void *stream);
/* The checks of gbx_mm_map_host on every offset array, and a region's read inside 0 .. n_reads - 1.  More text than text_cap:
 * GBX_ERR_ARG with the need in *n_text and gbx_last_error() (line_off is written; call with 0 / NULL to size). */
int gbx_mm_paf_host(int64_t n_reads, const gbx_mm_reg *regs, const int64_t *reg_off,
                    const uint8_t *qnames, const int64_t *qname_off, const int64_t *seq_off, const int32_t *rep_len,
                    int64_t n_targets, const uint8_t *tnames, const int64_t *tname_off, const int64_t *tseq_off,
                    uint8_t *lines, int64_t text_cap, int64_t *line_off, int64_t *n_text);

/* ------------------------------------------------------------------- mm align: base-level alignment of the regions (`-c`)
 * The dynamic programme between a region's anchors and beyond its ends, after minimap2's mm_align1 and ksw2's ksw_extd2:
 * two-piece affine gaps gap(l) = min(q + e l, q2 + e2 l), a band, z-drop on the extensions, gaps left-aligned on the forward
 * strand.  UNPINNED by a compiled reference; the rules are DESIGN 3.20, restated in tests/mm_align_ref.py.  In short:
 *   codes     A C G T in either case 0..3, anything else 4; s(t, c) = -sc_ambi if a code is above 3, a if equal, else -b
 *   a job     target T[0..tl) x query Q[0..ql), band w, ties LEFT or RIGHT, global or extension.  Cell (t, j) of antidiagonal
 *             r = t + j is in the band iff (r - w + 1) >> 1 <= t <= (r + w) >> 1; outside it everything is minus infinity.
 *             H(-1,-1) = 0, H(-1,j) = -gap(j + 1), H(t,-1) = -gap(t + 1), gap states on a border are minus infinity.
 *             E = max(H(t-1,j) - q, E(t-1,j)) - e (deletion), F likewise from (t,j-1) (insertion), E2 F2 with q2 e2; a state's
 *             continuation flag is set iff it extends (LEFT: E(t-1,j) > H(t-1,j) - q, RIGHT: >=; clear on a border).
 *             H = the diagonal plus s, then E F E2 F2 in that order, taken iff larger (LEFT) or not smaller (RIGHT).
 *             Extension: per antidiagonal the first largest H; z-drop when max - best > zdrop + l e2 beyond the maximum's cell;
 *             the end is the query-end cell when mqe + end_bonus > max and nothing dropped, else the maximum's cell, else empty.
 *             The walk back follows the cell's choice, a gap state while its flag at the cell it leaves is set.
 *   a region  breakpoints from its anchors: from (x0 + 1 - span0, y0 + 1 - span0), each next anchor gives re = max(x - (span >> 1),
 *             rs), qe likewise; a fill closes at the last anchor or once both sides reach min_ksw_len.  Fills are global LEFT jobs
 *             with w = max(bw, |tl - ql| + 1) (an empty side: one D or I), never z-dropped, so a region is never split.  Left
 *             extension: lq = min(qs, max_ext), lt = min(rs, lq + bw), both sequences reversed, RIGHT; right extension forward, LEFT.
 *   output    CIGAR words len << 4 | op (M 0, I 1, D 2) left + fills + right, equal neighbours merged; mlen, blen, n_ambi,
 *             nm = blen - mlen + n_ambi, dp_max and dp_score from the final CIGAR and the jobs' scores.
 * Bounds: penalties and the match score at most 255 each, reads and contigs shorter than 2^28 bases, so no CIGAR run reaches
 * 2^28.  Scores are 32-bit and anything at or below -2^29 counts as minus infinity: a job is exact while its largest penalty
 * times (tl + ql) stays below 2^29 (with the defaults: tl + ql below 2^26); beyond that it is not.
 * A region's CIGAR has at most 2 qlen + 1 words (every M or I run takes a query base, D runs lie between them), which sizes
 * cigar_cap without a counting call.  z takes about 2 (bw + 1) bytes a read base (a direction byte a band cell, and the rows):
 * about 1 000 at the default band, so one call aligns what its z room holds - the entries do not batch; a caller with more
 * reads than that calls once a batch.
 * Not modelled: splitting at a z-drop inside a fill, inversions, mm_fix_bad_ends, mm_filter_bad_seeds, long-join bands,
 * limiting an extension by the neighbouring region, the re-run of parents / selection / mapq on DP scores. */
typedef struct gbx_mm_align_params {
    int32_t a, b, sc_ambi;     /* 2, 4, 1 */
    int32_t q, e, q2, e2;      /* 4, 2, 24, 1 */
    int32_t bw;                /* 500 */
    int32_t zdrop;             /* 400; < 0: off */
    int32_t end_bonus;         /* 0 */
    int32_t min_ksw_len;       /* 200 */
    int32_t max_ext;           /* 5000 */
} gbx_mm_align_params;
#define GBX_MM_ALN_ALIGNED   1   /* flags of gbx_mm_aln */
#define GBX_MM_ALN_ZDROP_L   2
#define GBX_MM_ALN_ZDROP_R   4
#define GBX_MM_ALN_END_L     8
#define GBX_MM_ALN_END_R     16
#define GBX_MM_ALN_NO_ROOM   32  /* its jobs' direction bytes did not fit z_bytes: not aligned */
#define GBX_MM_ALN_INVALID   64  /* not aligned */
/* One per region, parallel to the regions: 56 bytes.  A region that is not aligned copies rs re qs qe mlen blen from its
 * gbx_mm_reg and has n_cigar = 0 and the rest 0. */
typedef struct gbx_mm_aln {
    int32_t rs, re, qs, qe;    /* qs, qe mirrored in qlen on the reverse strand, as gbx_mm_reg's */
    int32_t mlen, blen, n_ambi, nm;
    int32_t dp_score, dp_max;
    int32_t n_cigar, flags;
    int64_t cigar_off;         /* its words: cigar[cigar_off .. cigar_off + n_cigar) */
} gbx_mm_aln;

void gbx_mm_align_default_params(gbx_mm_align_params *p);
/* GBX_ERR_ARG naming the field: a < 1, a negative b / sc_ambi / q / q2 / end_bonus, e < 1, e2 < 1, bw < 1, min_ksw_len < 1,
 * max_ext < 0, a score or penalty above 255. */
int gbx_mm_align_check_params(const gbx_mm_align_params *p);

/* Alignment of the regions of gbx_mm_map_device (regs, its counts + 1 as d_n_regs, off / cax / cay / n_chained as it left
 * them) over the reads' text (seq, seq_off) and the contigs' (tseq, tseq_off[n_targets + 1]).  Output:
 *   alns[reg_cap]       one record a region
 *   cigar[cigar_cap]    the regions' words, region after region
 *   counts[3]           jobs (left, fills, right of every valid region), CIGAR words, bytes of z needed
 * d_z: z_bytes of room for the jobs' direction bytes and DP rows, 16-aligned, handed out in region order: a region whose jobs
 * end past z_bytes is not aligned (flag 32) and counts[2] reports what all of them need.  More words than cigar_cap: nothing is
 * written past it, counts[1] reports the need, and the statistics of a region whose words do not all fit are 0.  The device
 * entry does no host synchronisation. */
size_t gbx_mm_align_workspace_bytes(int64_t n_reads, int64_t reg_cap, int64_t anchor_cap);
int gbx_mm_align_device(const gbx_mm_align_params *p, int64_t n_reads, const gbx_mm_reg *d_regs, const int64_t *d_reg_off, const int64_t *d_n_regs,
                        int64_t reg_cap, const int64_t *d_off, const uint64_t *d_cax, const uint64_t *d_cay, const int32_t *d_n_chained,
                        int64_t anchor_cap, const uint8_t *d_seq, const int64_t *d_seq_off, int64_t n_targets, const uint8_t *d_tseq,
                        const int64_t *d_tseq_off, gbx_mm_aln *d_alns, uint32_t *d_cigar, int64_t cigar_cap, int64_t *d_counts,
                        void *d_z, int64_t z_bytes, void *d_work, size_t work_bytes, void *stream);
/* Host buffers in and out.  Checked before the device is touched, GBX_ERR_ARG naming the lowest offender: null pointers, offsets
 * that do not start at 0 or decrease, negative capacities, a region whose read is not the one reg_off puts it in, n_chained
 * outside its read's anchors; GBX_ERR_UNSUPPORTED: more than GBX_MM_MAX_READS reads, a read or contig of 2^28 bases or more.
 * More words than cigar_cap, or a region left with flag 32: GBX_ERR_ARG with the needs in counts[3] (call with cigar_cap 0 /
 * z_bytes 0 / NULL to size; alns is written). */
int gbx_mm_align_host(const gbx_mm_align_params *p, int64_t n_reads, const gbx_mm_reg *regs, const int64_t *reg_off,
                      const int64_t *off, const uint64_t *cax, const uint64_t *cay, const int32_t *n_chained,
                      const uint8_t *seq, const int64_t *seq_off, int64_t n_targets, const uint8_t *tseq, const int64_t *tseq_off,
                      gbx_mm_aln *alns, uint32_t *cigar, int64_t cigar_cap, int64_t z_bytes, int64_t *counts);

/* PAF text with CIGAR: an aligned region prints qname qlen qs qe +/- tname tlen rs re mlen blen mapq NM:i: ms:i: AS:i: nn:i:
 * tp:A: cm:i: s1:i: s2:i: (primaries) rl:i: cg:Z: with the coordinates and lengths of its gbx_mm_aln; one that is not aligned
 * prints the line of gbx_mm_paf_*.  Otherwise the contract of gbx_mm_paf_*, with a workspace size of its own. */
size_t gbx_mm_paf_cigar_workspace_bytes(int64_t n_reads, int64_t reg_cap);
int gbx_mm_paf_cigar_device(int64_t n_reads, const gbx_mm_reg *d_regs, const int64_t *d_reg_off, const int64_t *d_n_regs, int64_t reg_cap,
                            const gbx_mm_aln *d_alns, const uint32_t *d_cigar, int64_t cigar_cap,
                            const uint8_t *d_qnames, const int64_t *d_qname_off, const int64_t *d_seq_off, const int32_t *d_rep_len,
                            int64_t n_targets, const uint8_t *d_tnames, const int64_t *d_tname_off, const int64_t *d_tseq_off,
                            uint8_t *d_lines, int64_t text_cap, int64_t *d_line_off, int64_t *d_n_text, void *d_work, size_t work_bytes, void *stream);
int gbx_mm_paf_cigar_host(int64_t n_reads, const gbx_mm_reg *regs, const int64_t *reg_off, const gbx_mm_aln *alns, const uint32_t *cigar,
                          int64_t n_cigar, const uint8_t *qnames, const int64_t *qname_off, const int64_t *seq_off, const int32_t *rep_len,
                          int64_t n_targets, const uint8_t *tnames, const int64_t *tname_off, const int64_t *tseq_off,
                          uint8_t *lines, int64_t text_cap, int64_t *line_off, int64_t *n_text);

/* ------------------------------------------------------------------- mm sam: SAM records, cs / MD tags and = / X operations
 * The text of the aligned regions behind gbx_mm_align_*, beside gbx_mm_paf_cigar_*.  UNPINNED by a compiled reference; the rules
 * are DESIGN 3.21, restated in tests/mm_sam_ref.py, after minimap2's mm_write_sam3, write_cs_core, write_MD_core and
 * mm_update_cigar_eqx.  In short:
 *   columns   codes as mm align's; two columns are equal iff their codes are (4 against 4 is equal).  The alignment lies between
 *             the contig forward and the read as the anchors see it: reversed and complemented (ACGTUMRWSYKVHDBN ->
 *             TGCAAKYWSRMBDHVN, case kept, other bytes as they are) on the reverse strand.
 *   prints    a region prints its alignment iff gbx_mm_paf_cigar_* prints its cg:Z: line.  Any other region prints the plain PAF
 *             line (format 0) or nothing (format 1, counted in counts[1]).
 *   eqx       every M word is cut into maximal runs of equal (=, op 7) and unequal (X, op 8) columns; letters MIDNSHP=X.
 *   cs        short: `:n` a maximal equal run within an M word, `*` contig letter read letter (acgtn) an unequal column, `+` and the
 *             read letters an I, `-` and the contig letters a D.  Long: `=` and the letters (ACGTN) in place of `:n`.
 *   MD        a counter over equal M columns, printed with the contig letter (ACGTN) at an unequal column and with `^` and the
 *             contig letters at a D, each of which resets it; an I leaves it alone; at the end it prints only when above 0.
 *   SAM       QNAME FLAG RNAME rs+1 mapq CIGAR * 0 0 SEQ QUAL, the tags NM ms AS nn tp cm s1 s2 rl of the PAF line, SA:Z:, cs:Z:,
 *             MD:Z:.  Among a read's printing regions the first with parent == id is the primary, the others with parent == id are
 *             supplementary (0x800), the rest secondary (0x100); 0x10 on the reverse strand.  Clips S, or H on supplementary and
 *             secondary records unless softclip; SEQ and QUAL `*` on secondary records, the oriented read between H clips, else
 *             the whole oriented read; QUAL mirrored, `*` without qual.  SA on every parent == id record of a read with two or
 *             more, the others as tname,rs+1,+|-,[c5 S]lM[dI|dD][c3 S],mapq,NM; with l = min(qe - qs, re - rs).  A read none of
 *             whose regions prints gives QNAME 4 * 0 0 * * 0 0 SEQ QUAL as stored.
 *   PAF       the line of gbx_mm_paf_cigar_*, with the = / X letters, cs:Z: and MD:Z: behind it as asked; with every field 0 the
 *             text is gbx_mm_paf_cigar_*'s byte for byte.
 * Malformed input is cut, never read past: a word counts at most to the end of the read (M, I) or the contig (M, D), an op above
 * 2 counts no columns, a word that counts none prints nothing in cs and MD, a region whose `read` is not the read reg_off puts it
 * in prints nothing. */
typedef struct gbx_mm_sam_params {
    int32_t format;            /* 0 PAF, 1 SAM */
    int32_t cs;                /* 0 none, 1 short, 2 long */
    int32_t md;                /* 0, 1 */
    int32_t eqx;               /* 0, 1 */
    int32_t softclip;          /* 0, 1: S clips on supplementary and secondary records */
} gbx_mm_sam_params;

void gbx_mm_sam_default_params(gbx_mm_sam_params *p);          /* every field 0 */
/* GBX_ERR_ARG naming the field: a value outside the ones listed above. */
int gbx_mm_sam_check_params(const gbx_mm_sam_params *p);

/* The arguments of gbx_mm_paf_cigar_device, the parameters, the reads' bytes (seq on seq_off), their qualities on the same
 * offsets (qual, may be NULL) and the contigs' text (tseq on tseq_off).  Output: lines, line_off[n_reads + 1], *n_text as
 * gbx_mm_paf_*'s, counts[2] = lines written (as if text_cap held them all), regions that print nothing.  Nothing is written at or
 * past text_cap, *n_text reports the true need.  No host synchronisation. */
size_t gbx_mm_sam_workspace_bytes(int64_t n_reads, int64_t reg_cap);
int gbx_mm_sam_device(const gbx_mm_sam_params *p, int64_t n_reads, const gbx_mm_reg *d_regs, const int64_t *d_reg_off, const int64_t *d_n_regs,
                      int64_t reg_cap, const gbx_mm_aln *d_alns, const uint32_t *d_cigar, int64_t cigar_cap,
                      const uint8_t *d_qnames, const int64_t *d_qname_off, const uint8_t *d_seq, const uint8_t *d_qual, const int64_t *d_seq_off,
                      const int32_t *d_rep_len, int64_t n_targets, const uint8_t *d_tnames, const int64_t *d_tname_off, const uint8_t *d_tseq,
                      const int64_t *d_tseq_off, uint8_t *d_lines, int64_t text_cap, int64_t *d_line_off, int64_t *d_n_text, int64_t *d_counts,
                      void *d_work, size_t work_bytes, void *stream);
/* The checks of gbx_mm_paf_cigar_host.  More text than text_cap: GBX_ERR_ARG with the need in *n_text (line_off and counts are
 * written; call with 0 / NULL to size). */
int gbx_mm_sam_host(const gbx_mm_sam_params *p, int64_t n_reads, const gbx_mm_reg *regs, const int64_t *reg_off, const gbx_mm_aln *alns,
                    const uint32_t *cigar, int64_t n_cigar, const uint8_t *qnames, const int64_t *qname_off, const uint8_t *seq, const uint8_t *qual,
                    const int64_t *seq_off, const int32_t *rep_len, int64_t n_targets, const uint8_t *tnames, const int64_t *tname_off,
                    const uint8_t *tseq, const int64_t *tseq_off, uint8_t *lines, int64_t text_cap, int64_t *line_off, int64_t *n_text,
                    int64_t *counts);

#ifdef __cplusplus
}
#endif
#endif /* GBX_H */
