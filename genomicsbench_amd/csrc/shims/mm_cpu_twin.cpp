// mm_cpu_twin.cpp — the device's minimizer machine (mm_machine.h) compiled for the host: libgbx_mm_cpu.so.  One thread.  The
// tests run it in pieces against the plain-Python restatement (the warm start is exact), scripts/time_mm_seed.py times it.
#include <vector>
#include "../mm_machine.h"

namespace {
struct Ring {
    uint64_t bx[256], by[256];
    int bq[gbx::MM_TQ];
    uint64_t &x(int j) { return bx[j]; }
    uint64_t &y(int j) { return by[j]; }
    int &q(int j) { return bq[j]; }
};
struct Emit {
    uint64_t *ox, *oy;
    int64_t cap, n;
    void operator()(uint64_t x, uint64_t y) { if (n < cap) { ox[n] = x; oy[n] = y; } ++n; }
};
}  // namespace

extern "C" {

// The minimizers of one sequence, taken in pieces of `chunk` bases (0: the whole sequence at once) -> their number; the first
// cap of them are written.
int64_t gbx_mm_cpu_sketch(const uint8_t *seq, int64_t len, int w, int k, uint32_t rid, int is_hpc, int64_t chunk, uint64_t *ox, uint64_t *oy,
                          int64_t cap)
{
    Ring ring;
    Emit emit{ox, oy, cap, 0};
    if (len <= 0) return 0;
    if (chunk <= 0) chunk = len;
    for (int64_t lo = 0; lo < len; lo += chunk)
        gbx::mm_sketch_piece(seq, len, w, k, rid, is_hpc != 0, lo, lo + chunk < len ? lo + chunk : len, ring, emit);
    return emit.n;
}

}  // extern "C"
