// capi_common.h — what every capi_<kernel>.hip includes: the internal declarations, the host entries' transfer pipeline
// (host_pipeline.h), the bwa-mem entries' shared checks (host_mem.h), the multi-device layer on top of it (host_multi.h), the call combiner (host_combine.h) and the device
// allocations kept between calls (host_cache.h).
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "gbx_internal.h"

namespace gbx {
int require_device();      // GBX_OK, or GBX_ERR_NO_DEVICE with the error text set (gbx_core.hip)
}

#include "host_pipeline.h"
#include "host_mem.h"
#include "host_multi.h"
#include "host_combine.h"
#include "host_cache.h"

namespace gbx {
// Several small arrays out of one device block: a lane keeps at most 48 idle blocks between calls (host_pipeline.h), and the one
// call would hold more than that with a block per array.
struct Carve {
    DevBuf buf;
    size_t need = 0, used = 0;
    explicit Carve(Lane *l) : buf(l) {}
    void want(size_t bytes) { need += (bytes + 255) & ~(size_t)255; }
    int alloc() { return buf.alloc(need); }
    template <class T> T *take(size_t bytes) { T *p = (T *)((char *)buf.p + used); used += (bytes + 255) & ~(size_t)255; return p; }
};

// where the reference exits or asserts (meth.c:54-58, 65-68, 135), before any device work
inline int check_cigars(const char *who, int64_t n_reads, const int64_t *cigar_off, const uint32_t *cigar, const int32_t *seq_len)
{
    if (cigar_off[0] < 0) { set_error("%s: cigar_off below 0", who); return GBX_ERR_ARG; }
    for (int64_t r = 0; r < n_reads; ++r) {
        if (cigar_off[r + 1] < cigar_off[r]) { set_error("%s: cigar_off not monotone at read %lld", who, (long long)r); return GBX_ERR_ARG; }
        if (cigar_off[r + 1] > cigar_off[r] && !cigar) { set_error("%s: null pointer", who); return GBX_ERR_ARG; }
        if (seq_len[r] < GBX_ABEA_KMER) { set_error("%s: read %lld needs at least %d bases", who, (long long)r, GBX_ABEA_KMER); return GBX_ERR_ARG; }
        int64_t aligned = 0, advance = 0;
        for (int64_t c = cigar_off[r]; c < cigar_off[r + 1]; ++c) {
            const int op = (int)(cigar[c] & 0xf);
            const int64_t len = cigar[c] >> 4;
            if (op == 3) { set_error("%s: read %lld: a spliced alignment (operation N)", who, (long long)r); return GBX_ERR_ARG; }
            if (op == 6 || op > 8) { set_error("%s: read %lld: unhandled CIGAR operation %d", who, (long long)r, op); return GBX_ERR_ARG; }
            if (op == 0 || op == 7 || op == 8) aligned += len;
            if (op != 5) advance += len;
        }
        if (aligned > seq_len[r]) {
            set_error("%s: read %lld: %lld aligned bases, the read has %d", who, (long long)r, (long long)aligned, seq_len[r]);
            return GBX_ERR_ARG;
        }
        if (advance > 0x3fffffffLL) { set_error("%s: read %lld: its CIGAR spans more than 2^30 positions", who, (long long)r); return GBX_ERR_UNSUPPORTED; }
    }
    return GBX_OK;
}

// calculate_transitions (hmm.c:212-295, eventalign.c:171-240; the two are the same lines) for a read: lp_mk mb mm_self mm_next bb
// bk bm_next bm_self kk km.  Host C library, so that the logarithms carry the reference's bits.
inline void abea_transitions(double events_per_base, float *t)
{
    float p_stay = 1 - (1 / events_per_base);
    float p_skip = 0.0025, p_bad = 0.001, p_bad_self = p_bad, p_skip_self = 0.3;
    float p_mk = p_skip, p_mb = p_bad, p_mm_self = p_stay;
    float p_mm_next = 1.0f - p_mm_self - p_mk - p_mb;
    float p_bb = p_bad_self, p_bk, p_bm_next, p_bm_self;
    p_bk = p_bm_next = p_bm_self = (1.0f - p_bb) / 3;
    float p_kk = p_skip_self, p_km = 1.0f - p_kk;
    /* the reference's `log` has a float argument in C++: the float overload */
    t[0] = logf(p_mk); t[1] = logf(p_mb); t[2] = logf(p_mm_self); t[3] = logf(p_mm_next);
    t[4] = logf(p_bb); t[5] = logf(p_bk); t[6] = logf(p_bm_next); t[7] = logf(p_bm_self);
    t[8] = logf(p_kk); t[9] = logf(p_km);
}

// abea from raw signal, continued on the device (capi_abea_events.hip): what events -> scalings -> align() leave there for all
// n_reads reads, handed to `tail` on the lane's compute stream once align() is queued.  Absolute indexing throughout; a read
// without events has n_pairs 0.  The event records and the pairs are not downloaded.
struct AbeaAligned {
    Lane *L;
    int64_t n_reads, seq_bytes;
    const int64_t *event_off;                 // host, n_reads + 1
    const int32_t *n_pairs;                   // host, n_reads
    const int64_t *d_seq_off; const int32_t *d_seq_len; const char *d_seq;
    const int64_t *d_event_off; const float *d_event_mean; const gbx_abea_model *d_models;
    float *d_scale, *d_shift;
    const gbx_abea_pair *d_pairs;
    const gbx_abea_event *d_events;           // the 24-byte records, beside the means
};
typedef int (*abea_tail_fn)(void *ctx, const AbeaAligned &a);
int abea_signal_align_tail(const char *who, int64_t n_reads, const int16_t *raw, const int64_t *raw_off, const float *range, const float *digitisation,
                           const float *offset, const int64_t *seq_off, const int32_t *seq_len, const char *seq_arena, int64_t seq_bytes,
                           const gbx_abea_model *models, int32_t *status, float *scale, float *shift, abea_tail_fn tail, void *ctx);
}
