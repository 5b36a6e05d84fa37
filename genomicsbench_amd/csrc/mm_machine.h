// mm_machine.h — minimap2's minimizer machine (mm_sketch) on a stretch of one sequence, for the device (mm_kernels.hip) and for a
// plain C++ build on the host (scripts/time_mm_seed.py times it single-threaded).  The rules: DESIGN 3.18.
//
// A piece [lo, hi) of a sequence owns the steps that START in it (under HPC a step is a whole run of equal bases, and N is a
// step of its own); it pushes what those steps push.  The machine is started at fresh state w + k steps ahead of the step that
// holds lo (or at the sequence's start, whichever comes first), and what it pushes before lo is dropped: after w + k slots the
// ring, the minimum and every comparison l takes part in are those of the full run.  That holds for odd k only: a partly filled
// k-mer of an even k can equal its reverse complement, which is skipped without a slot, so for even k a piece is the whole
// sequence.  The piece with hi >= len flushes the last minimum.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define GBX_MM_HD __host__ __device__
#else
#define GBX_MM_HD
#endif

namespace gbx {

constexpr int MM_CHUNK = 256;                      // bases a piece owns (GBX_MM_SKETCH_CHUNK)
constexpr int MM_TQ = 32;                          // room for the run-length queue (k <= 28)

GBX_MM_HD inline int mm_code(uint8_t ch)
{
    const uint8_t u = ch & 0xdf;
    return u == 'A' ? 0 : u == 'C' ? 1 : u == 'G' ? 2 : u == 'T' ? 3 : 4;
}

GBX_MM_HD inline uint64_t mm_hash64(uint64_t key, uint64_t mask)
{
    key = (~key + (key << 21)) & mask;
    key = key ^ key >> 24;
    key = ((key + (key << 3)) + (key << 8)) & mask;
    key = key ^ key >> 14;
    key = ((key + (key << 2)) + (key << 4)) & mask;
    key = key ^ key >> 28;
    key = (key + (key << 31)) & mask;
    return key;
}

// the start of the step that holds position r (r itself without HPC or on an ambiguous base)
GBX_MM_HD inline int64_t mm_step_start(const uint8_t *seq, int64_t r, bool hpc)
{
    if (!hpc) return r;
    const int c = mm_code(seq[r]);
    if (c < 4)
        while (r > 0 && mm_code(seq[r - 1]) == c) --r;
    return r;
}

// Ring: x(j), y(j) the w slots, q(j) the MM_TQ run lengths, each a reference.  Emit: emit(x, y).
template <class Ring, class Emit>
GBX_MM_HD inline void mm_sketch_piece(const uint8_t *seq, int64_t len, int w, int k, uint32_t rid, bool hpc, int64_t lo, int64_t hi,
                                      Ring &ring, Emit &emit)
{
    const uint64_t NONE = ~0ull, mask = (1ull << 2 * k) - 1;
    const int shift1 = 2 * (k - 1);
    int64_t i = lo;
    if (lo > 0) {
        i = mm_step_start(seq, lo, hpc);
        for (int s = 0; s < w + k && i > 0; ++s) i = mm_step_start(seq, i - 1, hpc);
    }
    for (int j = 0; j < w; ++j) { ring.x(j) = NONE; ring.y(j) = NONE; }
    uint64_t f = 0, r = 0, min_x = NONE, min_y = NONE;
    int l = 0, buf_pos = 0, min_pos = 0, q_front = 0, q_count = 0;
    int64_t span = 0;
    for (; i < len; ++i) {
        if (i >= hi) break;
        const bool own = i >= lo;
        const int c = mm_code(seq[i]);
        uint64_t ix = NONE, iy = NONE;
        if (c < 4) {
            if (hpc) {
                int64_t run = 1;
                while (i + run < len && mm_code(seq[i + run]) == c) ++run;
                i += run - 1;
                const int at = q_front + q_count < MM_TQ ? q_front + q_count : q_front + q_count - MM_TQ;
                ring.q(at) = (int)(run < 0x7fffffff ? run : 0x7fffffff);
                ++q_count;
                span += run;
                if (q_count > k) {
                    span -= ring.q(q_front);
                    q_front = q_front + 1 < MM_TQ ? q_front + 1 : 0;
                    --q_count;
                }
            } else span = l + 1 < k ? l + 1 : k;
            f = (f << 2 | (uint64_t)c) & mask;
            r = r >> 2 | (uint64_t)(3 ^ c) << shift1;
            if (f == r) continue;
            const int z = f < r ? 0 : 1;
            ++l;
            if (l >= k && span < 256) {
                ix = mm_hash64(z ? r : f, mask) << 8 | (uint64_t)span;
                iy = (uint64_t)rid << 32 | (uint64_t)(uint32_t)i << 1 | (uint64_t)z;
            }
        } else { l = 0; q_front = q_count = 0; span = 0; }
        ring.x(buf_pos) = ix; ring.y(buf_pos) = iy;
        if (l == w + k - 1 && min_x != NONE && own) {
            for (int j = buf_pos + 1; j < w; ++j)
                if (min_x == ring.x(j) && ring.y(j) != min_y) emit(ring.x(j), ring.y(j));
            for (int j = 0; j < buf_pos; ++j)
                if (min_x == ring.x(j) && ring.y(j) != min_y) emit(ring.x(j), ring.y(j));
        }
        if (ix <= min_x) {
            if (l >= w + k && min_x != NONE && own) emit(min_x, min_y);
            min_x = ix; min_y = iy; min_pos = buf_pos;
        } else if (buf_pos == min_pos) {
            if (l >= w + k - 1 && min_x != NONE && own) emit(min_x, min_y);
            min_x = NONE;
            for (int j = buf_pos + 1; j < w; ++j)
                if (min_x >= ring.x(j)) { min_x = ring.x(j); min_y = ring.y(j); min_pos = j; }
            for (int j = 0; j <= buf_pos; ++j)
                if (min_x >= ring.x(j)) { min_x = ring.x(j); min_y = ring.y(j); min_pos = j; }
            if (l >= w + k - 1 && min_x != NONE && own) {
                for (int j = buf_pos + 1; j < w; ++j)
                    if (min_x == ring.x(j) && min_y != ring.y(j)) emit(ring.x(j), ring.y(j));
                for (int j = 0; j <= buf_pos; ++j)
                    if (min_x == ring.x(j) && min_y != ring.y(j)) emit(ring.x(j), ring.y(j));
            }
        }
        if (++buf_pos == w) buf_pos = 0;
    }
    if (hi >= len && min_x != NONE) emit(min_x, min_y);
}

}  // namespace gbx
