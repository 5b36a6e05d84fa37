// gbx_internal.h — shared declarations between the C-ABI translation unit and
// the per-kernel HIP files of libgbx.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <mutex>
#include <vector>
#include "../../include/gbx.h"
#include "dbg_plan.h"

namespace gbx {

// thread-local last-error text (gbx_core.hip)
void set_error(const char *fmt, ...);
int  hip_fail(hipError_t e, const char *what);

#define GBX_HIP(call)                                            \
    do {                                                         \
        hipError_t e_ = (call);                                  \
        if (e_ != hipSuccess) return gbx::hip_fail(e_, #call);   \
    } while (0)

// Optional per-kernel timing with HIP events on the launch stream (gbx_profile_*).
// A Stage brackets one kernel launch; it is a no-op unless profiling is on.
// roctx ranges (the reference's analogue: ITT pause/resume and task markers around its timed regions,
// bsw/main_banded.cpp:203-205,274-276,293-295).  GBX_ROCTX=1 loads librocprofiler-sdk-roctx.so (libroctx64.so as
// a fallback) on first use and brackets host-entry calls, H2D / D2H transfers and kernel launches with
// roctxRangePush/Pop on the calling thread, so that `rocprofv3 --marker-trace` shows them beside the kernels;
// unset, the constructor is one predictable branch.
struct RoctxRange {
    explicit RoctxRange(const char *name);
    ~RoctxRange();
    bool on_;
};

struct Stage {
    Stage(const char *name, hipStream_t s);
    ~Stage();
    int slot_;
    hipStream_t s_;
    RoctxRange range_;
};

// ---- loop guards (-DGBX_LOOP_GUARD: a diagnostic build of libgbx.so, scripts/build_guard.sh; round 5) --------------------------------
// A device loop whose trip count depends on data (traceback extensions, work-list walks, spin-waits between wavefronts) hangs the
// whole process if the data is ever not what the algorithm guarantees.  In the guard build every such loop counts down from a bound
// derived from its input sizes; a loop that hits it records (kernel, loop, unit) in a device word and leaves, and the launch function
// returns GBX_ERR_HIP with the record in the error text instead of the process dying in a "GPU Hang".  The product build carries only
// the bounds that are free (a comparison the loop makes anyway).
//   GBX_GUARD(var, bound)                   declares the counter (nothing in the product build)
//   GBX_GUARD_TRIP(var, kernel, loop, unit) true when the bound is exhausted (constant false in the product build)
//   GBX_GUARD_CHECK(what)                   in a launch function, after its launches: hipDeviceSynchronize() (the whole device, other
//                                           callers' streams included: the guard build is diagnostic only and its timings mean nothing), then a record becomes an error
enum { GBX_GK_BSW = 1, GBX_GK_CHAIN = 2, GBX_GK_PHMM = 3, GBX_GK_POA = 4, GBX_GK_ABEA = 5, GBX_GK_FMI = 6, GBX_GK_PILEUP = 8, GBX_GK_DBG = 9, GBX_GK_MEM = 10, GBX_GK_KMER_INDEX = 11 };
#ifdef GBX_LOOP_GUARD
namespace { __device__ unsigned long long gbx_guard_word; }      // one per translation unit
__device__ inline bool gbx_guard_report(int kernel, int loop, long long unit)
{
    atomicCAS(&gbx_guard_word, 0ull, 1ull << 63 | (unsigned long long)kernel << 56 | (unsigned long long)loop << 48 | ((unsigned long long)unit & 0xffffffffffffull));
    return true;
}
#define GBX_GUARD(var, bound) long long var = (long long)(bound)
#define GBX_GUARD_TRIP(var, kernel, loop, unit) (--(var) < 0 && gbx::gbx_guard_report((kernel), (loop), (long long)(unit)))
static inline int gbx_guard_check(const char *what)
{
    unsigned long long v = 0;
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpyFromSymbol(&v, HIP_SYMBOL(gbx_guard_word), sizeof(v));
    if (e != hipSuccess) return hip_fail(e, what);
    if (!v) return GBX_OK;
    const unsigned long long zero = 0;
    (void)hipMemcpyToSymbol(HIP_SYMBOL(gbx_guard_word), &zero, sizeof(zero));
    set_error("%s: loop guard hit: kernel %d, loop %d, unit %lld (a data-dependent device loop ran past the bound its inputs allow)", what,
              (int)(v >> 56 & 0x7f), (int)(v >> 48 & 0xff), (long long)(v & 0xffffffffffffull));
    return GBX_ERR_HIP;
}
#define GBX_GUARD_CHECK(what) do { const int grc_ = gbx::gbx_guard_check(what); if (grc_) return grc_; } while (0)
#else
#define GBX_GUARD(var, bound)
#define GBX_GUARD_TRIP(var, kernel, loop, unit) false
#define GBX_GUARD_CHECK(what) do { } while (0)
#endif

// Side streams for independent kernels of one call (the per-class kernels have long single-wave tails that
// overlap well).  fork(): the side streams wait for everything queued on `main`; join(): `main` waits for
// them.  One set per device, created on first use and shared by every caller on that device: the launch
// functions hold `mu` from fork() to join() (host enqueue time only), because the events are shared and two
// host threads recording them in between each other would wait on the wrong record.
struct SideStreams {
    static constexpr int N = 3;
    hipStream_t side[N];
    hipStream_t pre[2];                          // urgent streams for the passes that prepare a launch (bsw's pipelined chunks)
    hipEvent_t ev_fork, ev_join[N], ev_aux;      // ev_aux: a point on one side stream the others wait for (bsw: the lane sort)
    hipEvent_t ev_pre;                           // the other preparing pass (bsw: classify)
    hipEvent_t ev_aux_first;                     // an earlier point on ev_aux's stream (bsw: the lane sort's first group)
    std::mutex mu;
    int fork(hipStream_t main);
    int join(hipStream_t main);
};
int side_streams(SideStreams **out);

// ---- bsw (bsw_kernels.hip)
// A chunk of a pipelined host call (join_events set): what has to happen between its uploads and its kernels.  With it the
// launch puts these passes (unpacking, classify, the lane sort) on the urgent streams, waiting for `uploaded` only, and the
// chunk's kernels wait for them - not, as everything on the caller's stream would, for the previous chunk's kernels.
struct BswChunkPrep {
    hipEvent_t uploaded;                          // recorded on the copy stream behind the chunk's uploads
    const uint8_t *ref_packed, *qer_packed;       // 4-bit arenas to unpack (nullptr: the bytes were uploaded as they are)
    uint8_t *ref_bytes, *qer_bytes;
    int64_t lo_r, hi_r, lo_q, hi_q;
    int64_t rows_pairs;                           // pairs of the chunk that bsw_lane_takes() turns down, or an upper bound; -1: not counted
    // 0: one call does everything.  1: the preparing passes only, behind `uploaded` = the chunk's index arrays (returns 1 and
    // queues nothing if this chunk's launch cannot be split); 2: the kernels, behind `uploaded` = its bases.  ev_pre / ev_aux:
    // the caller's own events that tie the two calls together (the side streams' are shared by all callers of a device).
    int phase;
    hipEvent_t ev_pre, ev_aux;
    // How far the caller's byte arenas have been expanded so far (the call's watermarks, nullptr: [lo, hi) as given).  A chunk
    // the lane kernels take whole reads the packed images and expands nothing, so the next chunk that does need the bytes
    // expands from the watermark, not from its own lo: its pairs may lie in what an earlier, packed chunk brought up.
    int64_t *unp_r = nullptr, *unp_q = nullptr;
};
// Which pairs a launch of n pairs puts on the lane kernels (bsw_kernels.hip: lane_ok), for a host pass that counts the
// others: a launch that knows there are none leaves out the row-kernel classes, twenty-one near-empty launches.
struct BswLaneRule { int on, max_mat, qmax, limit; };
int bsw_lane_rule(const gbx_bsw_params *p, int64_t n, BswLaneRule *r);
static inline bool bsw_lane_takes(const BswLaneRule &r, int qlen, int tlen, int h0)
{
    return r.on && qlen >= 1 && qlen <= r.qmax && tlen >= 1 && h0 >= 0 && h0 + qlen * r.max_mat < r.limit;
}
size_t bsw_workspace_bytes(int64_t n);
// for the tests: the sorted lists of the last lane sort on a workspace (synchronises the device); the sort's tile in pairs
int bsw_debug_lane_lists(const void *d_work, int64_t n, int32_t *h_order, int32_t *h_row_first);
int bsw_lane_sort_tile();
int bsw_launch(const gbx_bsw_params *p, int64_t n,
               const uint8_t *d_ref, const uint8_t *d_qer,
               const int64_t *d_idr, const int64_t *d_idq,
               const int32_t *d_len1, const int32_t *d_len2, const int32_t *d_h0,
               gbx_bsw_result *d_out, void *d_work, size_t work_bytes, hipStream_t s,
               hipEvent_t *join_events = nullptr, const struct BswChunkPrep *prep = nullptr);

int bsw_unpack4(const uint8_t *d_packed, uint8_t *d_out, int64_t lo, int64_t hi, hipStream_t s);
int bsw_launch_direct(const gbx_bsw_params *p, int64_t n, int max_qlen,
                      const uint8_t *d_ref, const uint8_t *d_qer, const int64_t *d_idr, const int64_t *d_idq,
                      const int32_t *d_len1, const int32_t *d_len2, const int32_t *d_h0, gbx_bsw_result *d_out, hipStream_t s);

// ---- chain (chain_kernels.hip)
size_t chain_workspace_bytes(int64_t n_calls, int64_t n_anchors);
int chain_launch(int64_t n_calls, int64_t n_anchors, const int64_t *d_off,
                 const uint64_t *d_ax, const uint64_t *d_ay, const gbx_chain_call *d_hdr,
                 int32_t *d_score, int32_t *d_parent, int32_t *d_target, int32_t *d_peak,
                 void *d_work, size_t work_bytes, hipStream_t s);

int chain_read_evaluated(const void *d_work, int64_t *pairs, hipStream_t s);
int chain_read_job_stats(const void *d_work, int64_t n_calls, int64_t n_anchors, int64_t *jobs, int64_t *longest, hipStream_t s);
int poa_read_cells(const void *d_work, size_t slots_bytes, int64_t *cells, hipStream_t s);

// ---- fmi (fmi_kernels.hip)
size_t fmi_index_bytes(int64_t ref_seq_len);
int fmi_index_build(const gbx_fmi_index *idx, void *d_index, size_t index_bytes, hipStream_t s);
size_t fmi_workspace_bytes(int64_t n_reads, int32_t max_len, int32_t min_seed_len, int raw_cap = 0);
int fmi_launch(const gbx_fmi_index *idx, const void *d_index, const gbx_fmi_params *p, int64_t n_reads, int32_t max_len,
               const uint8_t *d_enc, const int64_t *d_read_off, const int32_t *d_read_len, gbx_fmi_smem *d_out, int64_t out_cap,
               int64_t *d_smem_off, int64_t *d_n_out, void *d_work, size_t work_bytes, hipStream_t s, int raw_cap = 0);
int fmi_read_extensions(const void *d_work, int64_t *ext, hipStream_t s);
int fmi_read_overflow(const void *d_work, int64_t *worst, hipStream_t s);
// the index scalars are consistent and ref_seq_len <= max_len (the caller has checked idx for null); else GBX_ERR_ARG
int fmi_index_check(const gbx_fmi_index *idx, int64_t max_len, const char *who);
// the device indexes and suffix-array samples the host entries keep between calls (host_cache.h; capi_fmi.hip, capi_fmi_sal.hip)
struct HostCache;
extern HostCache fmi_index_cache, fmi_sa_cache;
// the device index of idx on device dev (the current one) from fmi_index_cache, held until fmi_index_cache.unuse(*d_index)
int fmi_index_acquire(const gbx_fmi_index *idx, int dev, hipStream_t s, void **d_index);

// ---- fmi suffix-array lookup (fmi_sal_kernels.hip)
bool fmi_sa_wide(int64_t ref_seq_len);           // 64-bit samples and kernel: ref_seq_len >= 2^32, or GBX_FMI_WIDE=1
size_t fmi_sa_bytes(int64_t n_sa, int64_t ref_seq_len);
int fmi_sa_build(const gbx_fmi_sa *sa, int64_t ref_seq_len, void *d_sa, size_t sa_bytes, hipStream_t s);
size_t fmi_sal_workspace_bytes(int64_t smem_cap, int64_t pos_cap);
int fmi_sal_launch(const gbx_fmi_index *idx, const void *d_index, const gbx_fmi_sa *sa, const void *d_sa, const gbx_fmi_smem *d_smems,
                   const int64_t *d_n_smem, int64_t smem_cap, int32_t max_occ, int64_t *d_pos, int64_t pos_cap, int64_t *d_pos_off,
                   int64_t *d_n_pos, void *d_work, size_t work_bytes, hipStream_t s);
int fmi_sal_read_steps(const void *d_work, int64_t *steps, int64_t *max_steps, hipStream_t s);

// ---- FM index construction (mem_index_kernels.hip): suffix array by prefix doubling on radix sorts, BWT, checkpoints, samples
bool fmi_build_fits(int64_t l_pac);              // 1 <= l_pac and 2 l_pac + 1 <= 2^32 - 1 (32-bit positions and ranks)
size_t fmi_build_workspace_bytes(int64_t l_pac); // 0 when it does not fit
// d_info: int64[8] = count[0..4], sentinel_index, doubling rounds run, slots the first round sorted.  Synchronises s once a round.
int fmi_build_launch(const uint8_t *d_genome, int64_t l_pac, int32_t sa_compx, gbx_fmi_cp_occ *d_cp, int8_t *d_ms, uint32_t *d_ls, uint8_t *d_text,
                     int64_t *d_info, void *d_work, size_t work_bytes, hipStream_t s);
int fmi_build_rounds(int64_t *slots, int32_t cap, int32_t *n_rounds);     // of the calling thread's last fmi_build_launch
// the host checks of every build entry (capi_mem_index.hip); genome: host codes to check, or null when they are on the device
int fmi_build_check(const uint8_t *genome, int64_t l_pac, int32_t sa_compx, const char *who);

// ---- what the device pipelines share: the scan (mem_scan.hip; its pieces and the other device helpers: dev_prims.h) and the
// radix sort built on it (dev_sort.hip).  What only the bwa-mem stages share on the device is in mem_common.h.
// One exclusive scan over per-unit counts.  cnt holds nq quantities of n counts, n + 1 entries apart; each becomes its offsets
// (entry n: the total) in place.  Three launches: a block scan, one block per quantity over the block sums, an offset pass.
struct MemScanGuard { const int64_t *n; int64_t lo, hi; };      // n == nullptr: no guard; else the stage before it fits iff lo <= *n <= hi
struct MemScanJob {
    long long *cnt; int64_t n; int nq;              // nq: 1 or 2
    long long *bsum; int blocks;                    // [nq][blocks] scratch, blocks = mem_scan_blocks(n)
    int64_t *total[2];                              // where a quantity's total goes (nullptr: nowhere); -1 when a guard fails
    int64_t *off0;                                  // quantity 0's offsets are also copied here (nullptr: not)
    MemScanGuard guard[2];
};
void mem_scan_launch(const MemScanJob &job, hipStream_t s);
// Stable LSD radix sort of items (uint64_t a, V b), V = uint32_t or uint64_t, a digit of up to 8 bits a pass; a pass is three
// launches: block histograms, mem_scan_launch over 256 * blocks entries, scatter.  The items start in buffer 0.
constexpr int SORT_THREADS = 256, SORT_ITEMS = 16, SORT_TILE = SORT_THREADS * SORT_ITEMS;      // a thread's and a block's elements
inline long long sort_blocks(long long n) { const long long b = (n + SORT_TILE - 1) / SORT_TILE; return b > 0 ? b : 1; }
struct SortPass { int word, shift; uint32_t mask; };           // the digit: (word 0: a, 1: b, V = uint64_t only) >> shift & mask, mask <= 255
struct SortCount { const int64_t *dev; long long n; };         // dev null: n items; else *dev clipped to n.  The grid covers n
template <class V>
struct SortBufs { uint64_t *a[2]; V *b[2]; long long *hist, *hsum; };      // hist: 256 sort_blocks(n) + 1, hsum: mem_scan_blocks of that
template <class V>
int radix_sort(const SortBufs<V> &bufs, const SortCount &count, const SortPass *pass, int n_pass, hipStream_t s);      // -> the buffer with the result
struct Carver;                                                  // dev_prims.h
struct SortLayout { size_t o_a[2], o_b[2], o_hist, o_hsum; };   // of (uint64_t, uint64_t) items
SortLayout sort_layout(int64_t cap, Carver &carve);
SortBufs<uint64_t> sort_bufs(char *wb, const SortLayout &L);
// the CIGAR list past *n (below 0: 0), up to cap: zeroed seeds (len = 0 is no seed) with results of all -1
void mem_sel_tail_launch(gbx_bsw_seed *seeds, gbx_bsw_seed_result *res, int64_t cap, const int64_t *n, hipStream_t s);

// ---- seed chaining (mem_chain_kernels.hip)
struct MemChainIo {                  // the device arguments of gbx_mem_chain_device
    const gbx_fmi_smem *smems; const int64_t *n_smem; int64_t smem_cap; const int64_t *smem_off;
    const int64_t *pos; const int64_t *n_pos; int64_t pos_cap; const int64_t *pos_off;
    const int64_t *read_off; const int32_t *read_len;
    int64_t l_pac; int32_t n_contigs; const int64_t *contig_off;
    gbx_mem_chain *chains; int64_t chain_cap; int64_t *chain_off;
    gbx_bsw_seed *seeds; int64_t seed_cap; int32_t *l_rep; int64_t *n_chains, *n_seeds;
};
size_t mem_chain_workspace_bytes(int64_t n_reads, int64_t smem_cap, int64_t pos_cap);
int mem_chain_launch(const gbx_mem_chain_params *p, int64_t n_reads, const MemChainIo &io, void *d_work, size_t work_bytes, hipStream_t s);

// ---- CIGAR of extended seeds (mem_cigar_kernels.hip)
struct MemCigarIo {                  // the device arguments of gbx_mem_cigar_device
    const gbx_bsw_seed *seeds; const gbx_bsw_seed_result *res;
    const uint8_t *text; int64_t text_bytes; const uint8_t *qer; int64_t qer_bytes;
    int64_t l_pac; int32_t n_contigs; const int64_t *contig_off;
    gbx_mem_aln *alns; uint32_t *cigar; int64_t cigar_cap; int64_t *n_cigar;
};
size_t mem_cigar_fixed_bytes(int64_t n);                                    // the workspace without the direction room
size_t mem_cigar_record_z_bytes(const gbx_mem_cigar_params *p, int32_t lq, int32_t lt);
// host side of the record rules: 0 invalid (rid = -1), 1 valid, -1 a range outside its arena; *z_need = its direction room
int mem_cigar_record_host(const gbx_mem_cigar_params *p, const gbx_bsw_seed &s, const gbx_bsw_seed_result &r, int64_t text_bytes,
                          int64_t qer_bytes, int64_t l_pac, size_t *z_need);
int mem_cigar_launch(const gbx_mem_cigar_params *p, int64_t n, const MemCigarIo &io, void *d_work, size_t work_bytes, int64_t z_bytes,
                     hipStream_t s);

// ---- alignment regions (mem_regs_kernels.hip)
struct MemRegsIo {                   // the device arguments of gbx_mem_regs_device
    const gbx_mem_chain *chains; const int64_t *n_chains; int64_t chain_cap; const int64_t *chain_off;
    const gbx_bsw_seed *seeds; const int64_t *n_seeds; int64_t seed_cap;
    const gbx_bsw_seed_result *res; const int32_t *l_rep;
    gbx_mem_reg *regs; int64_t reg_cap; int64_t *reg_off; int64_t *n_regs;
    gbx_bsw_seed *sel_seeds; gbx_bsw_seed_result *sel_res; int64_t sel_cap; int64_t *n_sel;
};
size_t mem_regs_workspace_bytes(int64_t n_reads, int64_t seed_cap);
int mem_regs_launch(const gbx_mem_regs_params *p, int64_t n_reads, int64_t read_id0, const MemRegsIo &io, void *d_work, size_t work_bytes,
                    hipStream_t s);

// ---- paired-end (mem_pair_kernels.hip)
struct MemPairIo {                   // the device arguments of gbx_mem_pair_device
    const gbx_mem_reg *regs; const int64_t *reg_off; const int64_t *n_regs; int64_t reg_cap;
    const gbx_bsw_seed *sel_seeds; const gbx_bsw_seed_result *sel_res; int64_t sel_cap;
    const gbx_bsw_seed *seeds; int64_t seed_cap; const int32_t *l_rep;
    int64_t l_pac; int32_t n_contigs; const int64_t *contig_off;
    gbx_mem_pestat *pes; gbx_mem_pair *pairs; gbx_mem_reg *pregs;
    gbx_bsw_seed *psel_seeds; gbx_bsw_seed_result *psel_res; int64_t psel_cap; int64_t *n_psel;
};
size_t mem_pair_workspace_bytes(int64_t n_pairs, int64_t reg_cap, int32_t max_ins);
// pes_in: a host pointer to the caller's four records (passed to the kernels by value), or null for an estimate from the call
int mem_pair_launch(const gbx_mem_pair_params *p, int64_t n_pairs, int64_t pair_id0, const MemPairIo &io, const gbx_mem_pestat *pes_in,
                    void *d_work, size_t work_bytes, hipStream_t s, const gbx_mem_pestat *d_pes_in = nullptr);

// ---- mate rescue (mem_rescue_kernels.hip)
struct MemRescueIo {                 // the device arguments of gbx_mem_rescue_device
    const gbx_mem_reg *regs; const int64_t *reg_off; const int64_t *n_regs; int64_t reg_cap;
    const gbx_bsw_seed *seeds; int64_t seed_cap; const int32_t *l_rep;
    const int64_t *read_off; const int32_t *read_len;
    const uint8_t *text; int64_t text_bytes; const uint8_t *qer; int64_t qer_bytes;
    int64_t l_pac; int32_t n_contigs; const int64_t *contig_off;
    const gbx_mem_pestat *pes;
    gbx_mem_reg *xregs; int64_t xreg_cap; int64_t *xreg_off; int64_t *n_xregs;
    gbx_bsw_seed *xseeds; int64_t xseed_cap; int64_t *n_xseeds;
    gbx_bsw_seed *xsel_seeds; gbx_bsw_seed_result *xsel_res; int64_t xsel_cap; int64_t *n_xsel;
    gbx_mem_rescue_stat *stats;
};
size_t mem_rescue_workspace_bytes(int64_t n_pairs, int64_t reg_cap, int32_t max_matesw);
int mem_rescue_launch(const gbx_mem_rescue_params *p, int64_t n_pairs, int64_t pair_id0, const MemRescueIo &io, void *d_work, size_t work_bytes,
                      hipStream_t s);
// step 1 of the paired stage alone: d_pes[4] from the regions (mem_pair_kernels.hip); reads regs, reg_off, n_regs, reg_cap, l_pac of io
size_t mem_pestat_workspace_bytes(int32_t max_ins);
int mem_pestat_launch(const gbx_mem_pair_params *p, int64_t n_pairs, const MemPairIo &io, void *d_work, size_t work_bytes, hipStream_t s);

// ---- SAM records (mem_sam_kernels.hip)
struct MemSamIo {                    // the device arguments of gbx_mem_sam_device
    const gbx_mem_reg *regs; const int64_t *reg_off; const int64_t *n_regs; int64_t reg_cap;
    const gbx_mem_pair *pairs;                      // mode 1
    const gbx_mem_aln *alns; int64_t n_alns; const uint32_t *cigar; const int64_t *n_cigar; int64_t cigar_cap;
    const uint8_t *qer; int64_t qer_bytes; const int64_t *read_off; const int32_t *read_len; const uint8_t *qual;
    const uint8_t *names; const int64_t *name_off; int64_t name_bytes;
    const uint8_t *cnames; const int64_t *cname_off; int64_t cname_bytes;
    const uint8_t *text; int64_t text_bytes; int64_t l_pac; int32_t n_contigs; const int64_t *contig_off;
    gbx_mem_sam_rec *recs; int64_t rec_cap; int64_t *rec_off; int64_t *n_recs;
    uint8_t *md; int64_t md_cap; int64_t *n_md;
    uint8_t *lines; int64_t text_cap; int64_t *n_text;
};
int64_t mem_sam_rec_max(int64_t n_reads, int64_t reg_cap, int64_t n_alns);      // the records a call can make at most
size_t mem_sam_workspace_bytes(int64_t n_reads, int64_t reg_cap, int64_t n_alns);
int mem_sam_launch(const gbx_mem_sam_params *p, int64_t n_reads, int mode, const MemSamIo &io, void *d_work, size_t work_bytes, hipStream_t s);

// ---- minimizer seeding in front of chain (mm_kernels.hip; the machine: mm_machine.h)
struct MmIndexView { int64_t *hdr; uint64_t *keys; int64_t *koff; uint64_t *vals; };      // hdr: n_vals, n_keys, mid_occ, k, w, is_hpc
MmIndexView mm_index_view(void *d_index, int64_t mini_cap);
size_t mm_index_bytes(int64_t mini_cap);
size_t mm_sketch_workspace_bytes(const gbx_mm_params *p, int64_t n_seqs, int64_t total_len);
int mm_sketch_launch(const gbx_mm_params *p, int64_t n_seqs, const uint8_t *d_seq, const int64_t *d_seq_off, int64_t total_len, int rid_ordinal,
                     uint64_t *d_mx, uint64_t *d_my, int64_t mini_cap, int64_t *d_mini_off, int64_t *d_n_mini, void *d_work, size_t work_bytes,
                     hipStream_t s);
size_t mm_index_workspace_bytes(const gbx_mm_params *p, int64_t n_seqs, int64_t total_len, int64_t mini_cap);
int mm_index_launch(const gbx_mm_params *p, int64_t n_seqs, const uint8_t *d_seq, const int64_t *d_seq_off, int64_t total_len, void *d_index,
                    int64_t mini_cap, void *d_work, size_t work_bytes, hipStream_t s);
struct MmSeedIo {                    // the device arguments of gbx_mm_seed_device
    const void *index; int64_t index_mini_cap, ref_n_seqs, ref_max_len;
    int64_t n_reads; const uint8_t *seq; const int64_t *seq_off; int64_t total_len;
    uint64_t *mini_x, *mini_y; int64_t mini_cap; int64_t *mini_off;
    uint64_t *ax, *ay; int64_t anchor_cap; int64_t *off; gbx_chain_call *hdr;
    int32_t *rep_len, *n_mini; int64_t *counts;
};
size_t mm_seed_workspace_bytes(const gbx_mm_params *p, int64_t n_reads, int64_t total_len, int64_t mini_cap, int64_t anchor_cap);
int mm_seed_launch(const gbx_mm_params *p, const MmSeedIo &io, void *d_work, size_t work_bytes, hipStream_t s);

// ---- minimap2 behind the chain scores (mm_map_kernels.hip; the rules: mm_map_rules.h)
struct MmMapIo {                     // the device arguments of gbx_mm_map_device
    int64_t n_reads; const int64_t *off; const uint64_t *ax, *ay; int64_t anchor_cap;
    const int32_t *f, *p, *v; const int64_t *seq_off; const int32_t *rep_len; const uint32_t *hash;
    int64_t *chain_off; uint64_t *u; int64_t chain_cap; uint64_t *cax, *cay; int32_t *n_chained;
    int64_t *reg_off; gbx_mm_reg *regs; int64_t reg_cap; int64_t *counts;
};
size_t mm_map_workspace_bytes(int64_t n_reads, int64_t anchor_cap, int64_t chain_cap);
int mm_map_launch(const gbx_mm_map_params *p, const MmMapIo &io, void *d_work, size_t work_bytes, hipStream_t s);
struct MmPafIo {                     // the device arguments of gbx_mm_paf_device and gbx_mm_paf_cigar_device
    int64_t n_reads; const gbx_mm_reg *regs; const int64_t *reg_off; const int64_t *n_regs; int64_t reg_cap;
    const gbx_mm_aln *alns; const uint32_t *cigar; int64_t cigar_cap;       // alns null: the plain text, no region prints cg:Z:
    const uint8_t *qnames; const int64_t *qname_off, *seq_off; const int32_t *rep_len;
    int64_t n_targets; const uint8_t *tnames; const int64_t *tname_off, *tseq_off;
    uint8_t *lines; int64_t text_cap; int64_t *line_off; int64_t *n_text;
};
size_t mm_paf_workspace_bytes(int64_t reg_cap);
int mm_paf_launch(const MmPafIo &io, void *d_work, size_t work_bytes, hipStream_t s);

// ---- base-level alignment of the regions (mm_align_kernels.hip; the rules: mm_align_rules.h)
struct MmAlignIo {                   // the device arguments of gbx_mm_align_device
    int64_t n_reads; const gbx_mm_reg *regs; const int64_t *n_regs; int64_t reg_cap;
    const int64_t *off; const uint64_t *cax, *cay; const int32_t *n_chained; int64_t anchor_cap;
    const uint8_t *seq; const int64_t *seq_off; int64_t n_targets; const uint8_t *tseq; const int64_t *tseq_off;
    gbx_mm_aln *alns; uint32_t *cigar; int64_t cigar_cap; int64_t *counts; uint8_t *z; int64_t z_bytes;
};
size_t mm_align_workspace_bytes(int64_t n_reads, int64_t reg_cap, int64_t anchor_cap);
int mm_align_launch(const gbx_mm_align_params *p, const MmAlignIo &io, void *d_work, size_t work_bytes, hipStream_t s);

// ---- SAM records, cs / MD and = / X of the aligned regions (mm_sam_kernels.hip; the rules: mm_sam_rules.h)
struct MmSamIo {                     // the device arguments of gbx_mm_sam_device: gbx_mm_paf_cigar_device's and the texts
    MmPafIo paf;
    const uint8_t *seq, *qual, *tseq;
    int64_t *counts;
};
size_t mm_sam_workspace_bytes(int64_t n_reads, int64_t reg_cap);
int mm_sam_launch(const gbx_mm_sam_params *p, const MmSamIo &io, void *d_work, size_t work_bytes, hipStream_t s);

// ---- the aligner's gather behind the chain (mem_align_kernels.hip): every stage's count into one record
struct MemAlignGather {              // a null pointer: the stage does not run, its count is 0
    const unsigned long long *fmi_counters;         // the fmi workspace: [2] is the slot overflow word fmi_read_overflow reads
    const int64_t *n_smem, *n_pos, *n_chains, *n_seeds, *n_regs, *n_sel, *n_xregs, *n_xseeds, *n_xsel, *n_psel, *n_cigar;
    const gbx_mem_aln *alns; int64_t n_alns;        // the CIGAR stage's records: rid == -2 and rid >= 0 are counted
    const int64_t *n_recs, *n_md, *n_text;
    gbx_mem_align_counts *out;
};
int mem_align_gather_launch(const MemAlignGather &g, hipStream_t s);

// ---- kmer (kmer_kernels.hip)
size_t kmer_workspace_bytes(int32_t k, int64_t n_reads);
int kmer_launch(const gbx_kmer_params *p, int64_t n_reads, const uint8_t *d_enc, const int64_t *d_read_off, const int32_t *d_read_len,
                gbx_kmer_stats *d_stats, int64_t *d_hist, uint64_t *d_sel_kmer, uint32_t *d_sel_count, int64_t sel_cap, void *d_work,
                size_t work_bytes, hipStream_t s);

// ---- kmer index (kmer_index_kernels.hip; the rules are in kmer_index_rules.h)
struct KmerIndexReads { const uint8_t *enc; const int64_t *read_off; const int32_t *read_len; int64_t n_reads, total_len; };
size_t kmer_index_workspace_bytes(int64_t n_reads, int64_t total_len, bool index);
int kmer_minimizers_launch(const gbx_kmer_index_params *p, const KmerIndexReads &rd, int64_t *d_mini_off, int32_t *d_mini_pos,
                           uint8_t *d_mini_rev, int64_t mini_cap, int64_t *d_n_mini, void *d_work, size_t work_bytes, hipStream_t s);
int kmer_index_launch(const gbx_kmer_index_params *p, const KmerIndexReads &rd, gbx_kmer_index_stats *d_stats, uint64_t *d_kmer,
                      int64_t *d_off, int64_t kmer_cap, uint64_t *d_pos, int64_t pos_cap, void *d_work, size_t work_bytes, hipStream_t s);

// ---- pileup (pileup_kernels.hip)
size_t pileup_workspace_bytes(int64_t n_reads, int64_t n_cigar, int64_t n_pos);
int pileup_layout_launch(const gbx_pileup_params *p, const gbx_pileup_reads *d, int64_t *d_pos_col, gbx_pileup_layout_stats *d_stats,
                         void *d_work, size_t work_bytes, hipStream_t s);
int pileup_count_launch(const gbx_pileup_params *p, const gbx_pileup_reads *d, const int64_t *d_pos_col, int64_t p0, int64_t p1,
                        int32_t *d_major, int32_t *d_minor, uint32_t *d_counts, void *d_work, size_t work_bytes, hipStream_t s);
// after a count launch: the lowest read whose entries it skipped for want of a dtype, or -1 (synchronises s)
int pileup_read_bad(const gbx_pileup_params *p, const gbx_pileup_reads *d, const void *d_work, int64_t *bad, hipStream_t s);

// ---- dbg (dbg_kernels.hip)
// The device inputs of a call: reads and window references (device pointers), rcp[r] = the occurrence slots of reads before r
// (max(0, l_seq - k - 1) each), ref_bytes: where the reads' byte addresses start in the kernels' one address space.
struct DbgDev {
    int32_t k, min_qual;
    int64_t ref_bytes;
    const uint8_t *ref, *seq, *qual;
    const int64_t *seq_off, *rcp;
    const uint16_t *flag;
};
// gbx_dbg_graph_*: where the nodes and edges of the call's windows go (nodes == nullptr: stats only); src values are moved
// by ref_shift / seq_shift (a shard's rebased arrays back to the caller's).
struct DbgGraphOut {
    gbx_dbg_node *nodes = nullptr;
    gbx_dbg_edge *edges = nullptr;
    const int64_t *node_off = nullptr, *edge_off = nullptr;
    int64_t ref_shift = 0, seq_shift = 0;
};
// batches of plan as dbg_cut_batches cuts them (dbg_plan.h, DbgWinPlan)
int dbg_launch(const DbgDev &a, const std::vector<DbgWinPlan> &plan, const std::vector<int64_t> &batches, DbgWinPlan *d_plan, int *d_err,
               char *d_region, gbx_dbg_stats *d_stats, const DbgGraphOut &g, hipStream_t s);

// ---- dbg_asm (dbg_asm_kernels.hip): cycle check, start list and path search on one range of windows whose graphs lie in
// nodes / edges at the capacities node_off / edge_off[nw + 1] (window j of the range: plan[j], plan[j].win its index in the call).
struct DbgAsmDev {
    int32_t nw, k, n_builds, last_round;          // last_round: k > k_last, a cyclic window is final as well
    gbx_dbg_asm_params ap;
    const DbgWinPlan *plan;
    const int64_t *node_off, *edge_off;
    const gbx_dbg_node *nodes;
    const gbx_dbg_edge *edges;
    const uint8_t *ref, *seq;
    int32_t *cyc;                                 // the call's windows: cyclic flag of the latest build
    int32_t *win_slot;                            // the call's windows: index in the range
    int32_t *deg, *list, *nxt;                    // node capacity of the range each (windows above DBG_ASM_LDS_NODES)
    int32_t *fin;                                 // nw: the window's graph is final
    int64_t *wstart;                              // nw
    int64_t *counters;                            // 0..2 the call's starts, paths, path nodes; 3 the range's first start
    int32_t *pathbuf;                             // path_blocks slices of path_slice ints
    int64_t path_slice;
    int32_t path_blocks;
    gbx_dbg_asm_out out;
};
constexpr int DBG_ASM_LDS_NODES = 4096;
int dbg_asm_launch(const DbgAsmDev &a, hipStream_t s);

// ---- phmm (phmm_kernels.hip)
size_t phmm_workspace_bytes(int64_t n_pairs, int64_t n_reads, int max_hap_len, int64_t stream_syms = -1);
int phmm_init_tables();
const float *phmm_host_mm_table_f(int *n);
int phmm_launch(int64_t n_pairs, const int32_t *pair_read, const int32_t *pair_hap,
                int64_t n_reads, const int64_t *read_off, const int32_t *read_len,
                const uint8_t *rs, const uint8_t *q, const uint8_t *qi, const uint8_t *qd, const uint8_t *qc,
                const int64_t *hap_off, const int32_t *hap_len, const uint8_t *hap, int max_hap_len,
                double *out, void *d_work, size_t work_bytes, hipStream_t s, int64_t stream_syms = -1);

// ---- abea (abea_kernels.hip)
size_t abea_workspace_bytes(int64_t n_reads, int64_t n_kmers_total, int64_t n_bands_total);
int abea_read_cells(const void *d_work, int64_t *cells, hipStream_t s);
// after abea_launch: the aligned pairs of all reads packed back to back (read r's n_pairs[r] pairs at d_prefix[r]) into the
// workspace's trace area, which is free by then; returns where
int abea_pack_pairs(int64_t n_reads, const int64_t *d_event_off, const gbx_abea_pair *d_out, const int32_t *d_n_pairs,
                    const int64_t *d_prefix, void *d_work, int64_t n_kmers_total, gbx_abea_pair **d_packed, hipStream_t s);
int abea_launch(int64_t n_reads, const int64_t *d_seq_off, const int32_t *d_seq_len, const char *d_seq,
                const int64_t *d_event_off, const float *d_event_mean, const gbx_abea_model *d_models,
                const float *d_scale, const float *d_shift, const int64_t *d_band_off, const int32_t *d_order,
                const double *d_lp, int64_t n_kmers_total, int64_t n_bands_total,
                gbx_abea_pair *d_out, int32_t *d_n_pairs, void *d_work, size_t work_bytes, hipStream_t s);

// ---- abea from raw signal (abea_events_kernels.hip)
int abea_events_launch(int pass, int64_t n_reads, const int16_t *d_raw, const int64_t *d_raw_off, const float *d_range,
                       const float *d_digitisation, const float *d_offset, int64_t *d_n_events, int64_t *d_event_off,
                       gbx_abea_event *d_events, float *d_event_mean, int64_t event_cap, int32_t *d_status, hipStream_t s);
int abea_scalings_launch(int64_t n_reads, const int64_t *d_seq_off, const int32_t *d_seq_len, const char *d_seq, const int64_t *d_event_off,
                         const float *d_event_mean, const gbx_abea_model *d_models, float *d_scale, float *d_shift, hipStream_t s);

// ---- abea methylation scoring (abea_meth_kernels.hip)
int abea_meth_launch(int64_t n_jobs, const gbx_abea_meth_job *d_jobs, const char *d_seq, const int64_t *d_event_off, const float *d_event_mean,
                     const float *d_scale, const float *d_shift, const float *d_var, const float *d_log_var, const gbx_abea_model *d_model,
                     const float *d_flogsum, const float *d_trans, const float *d_pre, const float *d_post, const int32_t *d_order,
                     const int64_t *class_off, float *d_scores, hipStream_t s);

// ---- abea call-methylation site planner and job order (abea_meth_plan_kernels.hip; the rules: abea_meth_rules.h)
size_t abea_meth_sites_work_bytes(int64_t n_reads);
int abea_meth_sites_launch(int pass, int64_t n_reads, const int64_t *d_ref_off, const int32_t *d_ref_len, const char *d_ref, const int32_t *d_ref_start_pos,
                           const uint8_t *d_rc, const int64_t *d_rec_off, const gbx_abea_pair *d_rec, void *d_work, int64_t *d_site_off, int64_t *d_byte_off,
                           uint8_t *d_bad, int64_t site_cap, gbx_abea_meth_site *d_sites, gbx_abea_meth_job *d_jobs, int64_t seq_cap, char *d_seq_arena,
                           hipStream_t s);
size_t abea_meth_order_work_bytes(int64_t n_jobs);
int abea_meth_order_launch(int64_t n_jobs, const gbx_abea_meth_job *d_jobs, int64_t seq_bytes, int64_t n_reads, const int64_t *d_event_off, int64_t flank_len,
                           int max_rows_bits, void *d_work, int32_t *d_order, int64_t *d_class_off, int64_t *d_first_bad, hipStream_t s);

// ---- abea methylation frequency, f5c meth-freq (abea_freq_kernels.hip; the rules: abea_freq_rules.h).  The arguments of the device entries
size_t abea_freq_work_bytes(int64_t n_in, int64_t n_items);
int abea_freq_launch(int pass, int64_t n_records, const gbx_abea_freq_record *d_records, const char *d_rec_arena, double threshold, int split_groups,
                     int pos_bits, int contig_bits, int64_t n_items, void *d_work, int64_t *d_item_off, int64_t *d_counts, int64_t site_cap,
                     gbx_abea_freq_site *d_sites, int64_t seq_cap, char *d_seq_arena, hipStream_t s);
int abea_freq_merge_launch(int pass, int64_t n_a, const gbx_abea_freq_site *d_sites_a, const char *d_arena_a, int64_t n_b, const gbx_abea_freq_site *d_sites_b,
                           const char *d_arena_b, int pos_bits, int contig_bits, void *d_work, int64_t *d_counts, int64_t site_cap,
                           gbx_abea_freq_site *d_sites, int64_t seq_cap, char *d_seq_arena, hipStream_t s);
size_t abea_freq_records_work_bytes(int64_t n_sites);
int abea_freq_records_launch(int pass, int64_t n_sites, const gbx_abea_meth_site *d_sites, const float *d_scores, int64_t n_reads, const int32_t *d_contig,
                             const int64_t *d_ref_off, const int32_t *d_ref_len, const char *d_ref, int32_t clip_start, int32_t clip_end, void *d_work,
                             int64_t *d_off, int64_t rec_cap, gbx_abea_freq_record *d_records, int64_t seq_cap, char *d_seq_arena, hipStream_t s);
size_t abea_freq_tsv_work_bytes(int64_t n_sites);
int abea_freq_tsv_launch(int pass, int64_t n_sites, const gbx_abea_freq_site *d_sites, const char *d_seq_arena, int64_t n_contigs, const int64_t *d_name_off,
                         const char *d_names, int header_kind, int with_header, void *d_work, int64_t *d_line_off, int64_t cap, char *d_out, hipStream_t s);

// ---- abea eventalign (abea_eventalign_kernels.hip)
struct AbeaEventalignArgs {                   // the device entry's arguments, by value to the kernel
    long long n_reads;
    const int64_t *seq_off; const int32_t *seq_len; const int64_t *event_off; const float *event_mean; const gbx_abea_model *models;
    const float *scale, *shift, *var, *log_var, *trans;
    const int32_t *map, *near, *flags;
    const int64_t *cigar_off; const uint32_t *cigar; const int32_t *pos; const uint8_t *rc;
    const int64_t *ref_off; const int32_t *ref_len; const char *ref;
    int32_t region_start, region_end;
    const int32_t *order;
    gbx_abea_eventalign_rec *rec; int32_t *n_rec; int32_t *status; int64_t *counts;
    long long n_cigar_total, rows_cap;
    void *work;
    float pre0;                               // pre_flank[0] = (float)log(1 - TRANS_START_TO_CLIP), eventalign.c:124
};
size_t abea_eventalign_workspace_bytes(int64_t n_reads, int64_t n_cigar_total, int64_t rows_cap);
int abea_eventalign_launch(AbeaEventalignArgs a, size_t work_bytes, hipStream_t s);

// ---- abea calibration and event-alignment record (abea_calib_kernels.hip)
int abea_calib_launch(int64_t n_reads, const int64_t *d_seq_off, const int32_t *d_seq_len, const char *d_seq, const int64_t *d_event_off,
                      const float *d_event_mean, const gbx_abea_model *d_models, const gbx_abea_pair *d_pairs, const int32_t *d_n_pairs,
                      float *d_scale, float *d_shift, float *d_var, double *d_var64, int32_t *d_map, double *d_events_per_base,
                      int32_t *d_n_event_alignment, int32_t *d_n_m_state, int32_t *d_flags, hipStream_t s);
int abea_record_launch(int pass, int64_t n_reads, const int64_t *d_cigar_off, const uint32_t *d_cigar, const int32_t *d_pos, const uint8_t *d_rc,
                       const int64_t *d_seq_off, const int32_t *d_seq_len, const int32_t *d_map, const int32_t *d_flags, int32_t *d_near,
                       int64_t *d_rec_off, gbx_abea_pair *d_rec, int64_t rec_cap, hipStream_t s);

// ---- poa (poa_kernels.hip)
constexpr int POA_PIPE_MAXLEN = 512;     // longest sequence of the pipelined DP (two-plane slots)
size_t poa_slot_bytes(int ncap, int deg, int lmax, bool long_slot);
size_t poa_workspace_bytes(const gbx_poa_plan *plan);
int poa_waves_per_cu(int ncap);
int poa_cu_count();                   // CUs of the current device (256 when it cannot be asked)
bool poa_scores_fit_int16(const gbx_poa_params *p, int64_t ncap, int lmax);
// int32 cells (poa_wide_kernel): windows whose scores may leave the int16 range, or whose graph outgrew what int16 admits
size_t poa_wide_slot_bytes(int ncap, int deg, int lmax);
size_t poa_wide_workspace_bytes(int ncap, int deg, int lmax, int n_slots);
int poa_launch_wide(const gbx_poa_params *p, int64_t n_windows, const int64_t *d_win_first_seq, const int64_t *d_seq_off, const int32_t *d_seq_len,
                    const uint8_t *d_arena, uint8_t *d_cons, int32_t *d_cons_len, int32_t *d_status, int64_t cons_stride,
                    int ncap, int deg, int lmax, int n_slots, void *d_work, size_t work_bytes, hipStream_t s);
int poa_launch(const gbx_poa_params *p, const gbx_poa_plan *plan, int64_t n_windows, const int64_t *d_win_first_seq, const int64_t *d_seq_off,
               const int32_t *d_seq_len, const uint8_t *d_arena,
               uint8_t *d_cons, int32_t *d_cons_len, int32_t *d_status, int64_t cons_stride,
               void *d_work, size_t work_bytes, hipStream_t s);

}  // namespace gbx
