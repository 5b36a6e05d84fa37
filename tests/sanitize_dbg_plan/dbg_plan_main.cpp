// dbg_plan_main.cpp — TEST-ONLY: the planner and the workspace layouts of genomicsbench_amd/csrc/dbg_plan.h driven under ASan +
// UBSan over seeded random window lists and the edges of tests/test_dbg_plan_cpu.py (no windows, empty windows first, last and in
// a row, a window at, under and over the table, 2^20 and 2^20 + 1 windows without slots, the assembly's area at the sizing
// function's least and at its full size).  Every plan must lie inside its tables and every range inside its area; prints
// "ok batches <n> ranges <n>".
#include <cstdio>
#include <cstdlib>
#include "../../genomicsbench_amd/csrc/dbg_plan.h"

using namespace gbx;

struct Call : DbgHostArrays {
    int64_t n_reads() const { return (int64_t)seq_off.size() - 1; }
    int64_t n_win() const { return (int64_t)ref_pos.size(); }
};

static uint64_t rng_state = 1;
static int64_t rnd(int64_t n)      // [0, n)
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (int64_t)((rng_state >> 33) % (uint64_t)n);
}

// empty: 0 none, 1 the first, 2 the last, 3 every window but each fifth, 4 all
static Call make_call(uint64_t seed, int64_t n_win, int64_t n_reads, int empty)
{
    rng_state = seed;
    Call c;
    c.seq_off.assign(1, rnd(9));
    for (int64_t r = 0; r < n_reads; ++r) c.seq_off.push_back(c.seq_off.back() + rnd(152));
    c.ref_off.assign(1, rnd(9));
    for (int64_t w = 0; w < n_win; ++w) {
        const bool e = empty == 4 || (empty == 1 && w == 0) || (empty == 2 && w == n_win - 1) || (empty == 3 && w % 5 != 0);
        const int64_t lo = rnd(n_reads + 1), hi = e ? lo : lo + rnd(std::min<int64_t>(n_reads - lo, 40) + 1);
        c.ref_off.push_back(c.ref_off.back() + (e ? rnd(5) : rnd(601)));
        c.ref_pos.push_back(rnd((int64_t)1 << 30));
        c.read_lo.push_back(lo);
        c.read_hi.push_back(hi);
    }
    return c;
}

static void fail(const char *what, long long a, long long b)
{
    std::printf("FAILED %s: %lld %lld\n", what, a, b);
    std::exit(1);
}

static long long n_batches = 0, n_ranges = 0;

static void batches(const Call &c, int k, int64_t w0, int64_t w1, size_t table)
{
    const std::vector<int64_t> rcp = dbg_read_prefix(k, c.n_reads(), c.seq_off.data());
    std::vector<DbgWinPlan> plan;
    std::vector<int64_t> cut;
    const int64_t bad = dbg_cut_batches(k, w0, w1, c, rcp.data(), table, plan, cut);
    if (bad >= 0) {
        if (dbg_window_bytes(dbg_win_plan(k, bad, c, rcp.data()).C) <= table)
            fail("a window refused that fits", bad, (long long)table);
        return;
    }
    if ((int64_t)plan.size() != w1 - w0 || cut.front() != 0 || cut.back() != (int64_t)plan.size()) fail("plan size", (long long)plan.size(), w1 - w0);
    for (size_t b = 0; b + 1 < cut.size(); ++b) {
        if (cut[b + 1] <= cut[b]) fail("empty batch", (long long)b, cut[b]);
        if (cut[b + 1] - cut[b] > DBG_BATCH_WINDOWS) fail("batch above the window cap", (long long)b, cut[b + 1] - cut[b]);
        int64_t cand = 0;
        size_t used = 0;
        for (int64_t j = cut[b]; j < cut[b + 1]; ++j) {
            const DbgWinPlan &P = plan[(size_t)j];
            if (P.cand0 != cand || (size_t)P.base != used || P.win != j) fail("cand0 / base / win", j, P.base);
            used += dbg_window_bytes(P.C);
            cand += P.C;
        }
        if (used > table) fail("batch outside the tables", (long long)used, (long long)table);
        ++n_batches;
    }
}

static void ranges(const Call &c, int k0, int k, const std::vector<int64_t> &S, size_t work_bytes)
{
    const std::vector<int64_t> rcp0 = dbg_read_prefix(k0, c.n_reads(), c.seq_off.data()), rcp = dbg_read_prefix(k, c.n_reads(), c.seq_off.data());
    const DbgAsmLayout L = dbg_asm_layout(c.n_win(), c.n_reads(), dbg_max_occ(k0, c, rcp0.data()));
    if (work_bytes < L.least || L.least > L.bytes) fail("workspace below the least", (long long)work_bytes, (long long)L.least);
    const size_t limit = dbg_area_bytes(L.least - L.area, work_bytes - L.area), area = work_bytes - L.area;
    DbgAsmRange r;
    for (size_t done = 0; done < S.size();) {
        const size_t from = done;
        done = dbg_asm_cut_range(k, S, done, c, rcp.data(), limit, r);
        if (done <= from || done - from != r.plan.size() || r.node_off.size() != r.plan.size() + 1) fail("no progress", (long long)from, (long long)done);
        const DbgAsmRangeLayout G = dbg_asm_range_layout(r.tables, r.node_off.back(), r.edge_off.back());
        if (G.bytes > area) fail("range outside the area", (long long)G.bytes, (long long)area);
        for (size_t j = 0; j < r.plan.size(); ++j) {
            const DbgWinPlan &P = r.plan[j];
            if (P.win != S[from + j] || (size_t)P.base + dbg_window_bytes(P.C) > r.tables || r.node_off[j + 1] - r.node_off[j] != 2 * P.C) fail("range plan", (long long)j, P.base);
        }
        ++n_ranges;
    }
}

static void drive(const Call &c, int k, bool light)
{
    const int64_t n = c.n_win();
    const std::vector<int64_t> rcp = dbg_read_prefix(k, c.n_reads(), c.seq_off.data());
    size_t big = 0, total = 0;
    for (int64_t w = 0; w < n; ++w) {
        const size_t b = dbg_window_bytes(dbg_win_plan(k, w, c, rcp.data()).C);
        big = std::max(big, b);
        total += b;
    }
    const size_t tables[] = {big, big + 1, 2 * big, (big + total) / 2, total, total + 1, big ? big - 1 : 0, big / 2, 0};
    if (light) batches(c, k, 0, n, total);       // the window cap cuts, not the tables
    for (size_t t : tables)
        if (!light) batches(c, k, 0, n, t);
    if (n > 2) batches(c, k, 1, n, big), batches(c, k, n / 3, n - 1, big), batches(c, k, n / 2, n / 2, big);
    const int64_t occ = dbg_max_occ(k, c, rcp.data());
    const DbgBuildLayout B = dbg_build_layout(n, c.n_reads(), occ);
    if (!(B.rcp < B.plan && B.plan < B.err && B.err < B.region && B.region + big <= B.bytes)) fail("build layout", (long long)B.region, (long long)B.bytes);
    const DbgAsmLayout L = dbg_asm_layout(n, c.n_reads(), occ);
    std::vector<int64_t> all, later;
    for (int64_t w = 0; w < n; ++w) {
        all.push_back(w);
        if (w % 3 != 1) later.push_back(w);
    }
    const size_t works[] = {L.least, L.bytes, L.least + 1, (L.least + L.bytes) / 2};
    if (light) ranges(c, k, k, all, L.bytes);
    for (size_t work : works)
        if (!light) ranges(c, k, k, all, work), ranges(c, k, std::min(64, k + 5), later, work);
}

int main()
{
    const int ks[4] = {3, 15, 31, 64};
    for (int s = 0; s < 40; ++s) drive(make_call(100 + (uint64_t)s, 5 + 37 * (s % 10), 200 + 50 * (s % 7), 0), ks[s % 4], false);
    drive(make_call(1, 0, 10, 0), 15, false);
    drive(make_call(2, 6, 0, 0), 15, false);
    drive(make_call(3, 1, 30, 0), 15, false);
    for (int e = 1; e <= 4; ++e) drive(make_call(10 + (uint64_t)e, 12, 100, e), 15, false);
    for (int64_t n : {(int64_t)1 << 20, ((int64_t)1 << 20) + 1}) {
        Call c;
        c.seq_off.assign(1, 0);
        c.ref_off.assign((size_t)n + 1, 0);
        c.ref_pos.assign((size_t)n, 0);
        c.read_lo.assign((size_t)n, 0);
        c.read_hi.assign((size_t)n, 0);
        drive(c, 15, true);
    }
    std::printf("ok batches %lld ranges %lld\n", n_batches, n_ranges);
    return 0;
}
