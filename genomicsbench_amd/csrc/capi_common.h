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
};
typedef int (*abea_tail_fn)(void *ctx, const AbeaAligned &a);
int abea_signal_align_tail(const char *who, int64_t n_reads, const int16_t *raw, const int64_t *raw_off, const float *range, const float *digitisation,
                           const float *offset, const int64_t *seq_off, const int32_t *seq_len, const char *seq_arena, int64_t seq_bytes,
                           const gbx_abea_model *models, int32_t *status, float *scale, float *shift, abea_tail_fn tail, void *ctx);
}
