// carver.h — workspace carving, for the device files (through dev_prims.h) and for the plain host compiler (dbg_plan.h).
#pragma once
#include <stddef.h>

namespace gbx {
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
// carves a workspace: carve(bytes) -> the offset of the next piece, 256-aligned; at: the bytes taken so far
struct Carver {
    size_t at = 0;
    size_t operator()(size_t bytes) { const size_t o = at; at += align256(bytes); return o; }
};
}  // namespace gbx
