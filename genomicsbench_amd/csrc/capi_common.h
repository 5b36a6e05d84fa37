// capi_common.h — what every capi_<kernel>.hip includes: the internal declarations, the host entries' transfer pipeline
// (host_pipeline.h), the bwa-mem entries' shared checks (host_mem.h), the multi-device layer on top of it (host_multi.h), the call combiner (host_combine.h), the device
// allocations kept between calls (host_cache.h), Carve, upload and StreamDrain, and behind them what the abea entries share (host_abea.h).
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

// room for `bytes` in b and the copy of src into it on s (none at zero bytes)
inline int upload(DevBuf &b, const void *src, size_t bytes, hipStream_t s)
{
    const int rc = b.alloc(bytes);
    if (rc) return rc;
    if (bytes) GBX_HIP(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, s));
    return GBX_OK;
}

// Declared after every host array that a queued copy uses: however the scope is left, the stream is drained before they die.
struct StreamDrain { hipStream_t s; ~StreamDrain() { (void)hipStreamSynchronize(s); } };
}

#include "abea_meth_rules.h"
#include "host_abea.h"
