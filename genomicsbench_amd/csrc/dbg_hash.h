// dbg_hash.h — the hash and the table sizing of dbg_kernels.hip, for the device and for the plain host compiler (no HIP header
// in that mode): tests/hostcheck/dbg_hash_check.cpp builds it with g++, so that the collision cases of tests/dbg_cases.py are
// held against the kernel's own idea of tag and home slot.
//   node  h = mix64(FNV-1a over the k bytes); the slot's key holds the tag h >> 41, the probe starts at h & (nc - 1)
//   edge  key = (start node slot + 1) << 8 | next byte; the probe starts at mix64(key) & (ec - 1)
//   sizes nc = the first power of two >= 2C + 1, ec = the first >= C + 1 (both >= 2), C the window's occurrence slots
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GBX_DBG_HD __host__ __device__ inline
#else
#define GBX_DBG_HD inline
#endif

namespace gbx {

constexpr uint64_t DBG_FNV_BASIS = 0xcbf29ce484222325ull, DBG_FNV_PRIME = 0x100000001b3ull;
constexpr int DBG_TAG_SHIFT = 41;            // a node key: tag << 41 | (byte address + 1)

GBX_DBG_HD uint64_t dbg_fnv_step(uint64_t h, uint64_t byte) { return (h ^ byte) * DBG_FNV_PRIME; }

GBX_DBG_HD uint64_t dbg_fnv(const uint8_t *s, int k)
{
    uint64_t h = DBG_FNV_BASIS;
    for (int j = 0; j < k; ++j) h = dbg_fnv_step(h, s[j]);
    return h;
}

GBX_DBG_HD uint64_t dbg_mix64(uint64_t h)
{
    h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull; h ^= h >> 33;
    return h;
}

GBX_DBG_HD uint64_t dbg_node_tag(uint64_t h) { return h >> DBG_TAG_SHIFT; }
GBX_DBG_HD uint64_t dbg_node_home(uint64_t h, int64_t nc) { return h & ((uint64_t)nc - 1); }

GBX_DBG_HD uint64_t dbg_edge_key(int64_t slot, uint8_t byte) { return (uint64_t)(slot + 1) << 8 | byte; }
GBX_DBG_HD uint64_t dbg_edge_home(uint64_t key, int64_t ec) { return dbg_mix64(key) & ((uint64_t)ec - 1); }

GBX_DBG_HD int64_t dbg_node_slots(int64_t C)
{
    int64_t nc = 2;
    while (nc < 2 * C + 1) nc <<= 1;
    return nc;
}

GBX_DBG_HD int64_t dbg_edge_slots(int64_t C)
{
    int64_t ec = 2;
    while (ec < C + 1) ec <<= 1;
    return ec;
}

}  // namespace gbx
