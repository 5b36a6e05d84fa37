// dbg_plan.h — the planning rules of the dbg family, for the HIP files and for the plain host compiler (no HIP header):
// tests/hostcheck/dbg_plan_check.cpp builds it with g++ and tests/test_dbg_plan_cpu.py holds it against a restatement.
// The build cuts a call's windows into batches that fit its table region, the assembly cuts the windows still to do into ranges
// that fit its area; the layouts say where the pieces of the two workspaces lie, for the sizing entries, the "workspace too
// small" checks and the runs' pointers alike.
#pragma once
#include <algorithm>
#include <vector>
#include "../../include/gbx.h"
#include "carver.h"
#include "dbg_hash.h"

namespace gbx {

// One window of a batch or range: C occurrence slots from cand0 in the batch, nref_c of them the reference's; its tables at
// base in the batch region, nc node slots and ec edge slots (powers of two); win its index in the call's outputs.
struct DbgWinPlan { int64_t cand0, C, nref_c, base, nc, ec, read_lo, read_hi, ref_off, ref_pos, win; };
// A batch's tables or a range's graphs: at most this much device memory, or one window's if that alone is more.
constexpr size_t DBG_AREA_BYTES = (size_t)2 << 30;
constexpr int64_t DBG_BATCH_WINDOWS = 1 << 20;      // windows of one batch or range at most
// The assembly's searches' current paths: at most this much, 1024 wavefronts, at least one.
constexpr size_t DBG_ASM_PATH_BYTES = (size_t)256 << 20;
constexpr int DBG_ASM_PATH_BLOCKS = 1024;

// the occurrence slots of a sequence of len bytes; rcp[r] = those of the reads before r; those of a window with ref_len
// reference bytes and the reads [read_lo, read_hi)
inline int64_t dbg_seq_slots(int64_t len, int64_t k) { return std::max<int64_t>(0, len - k - 1); }
inline std::vector<int64_t> dbg_read_prefix(int k, int64_t n, const int64_t *seq_off)
{
    std::vector<int64_t> rcp((size_t)n + 1, 0);
    for (int64_t r = 0; r < n; ++r) rcp[(size_t)r + 1] = rcp[(size_t)r] + dbg_seq_slots(seq_off[r + 1] - seq_off[r], k);
    return rcp;
}
inline int64_t dbg_window_occ(int64_t k, int64_t ref_len, const int64_t *rcp, int64_t read_lo, int64_t read_hi) { return dbg_seq_slots(ref_len, k) + rcp[read_hi] - rcp[read_lo]; }

// The host's copies of a call's offsets and ranges, which the planners read: a host entry's, rebased, or a device entry's, read back.
struct DbgHostArrays { std::vector<int64_t> seq_off, ref_off, ref_pos, read_lo, read_hi; };
// window w's plan but for its place in a batch (base, cand0) and in the outputs (win), which the cutters give
inline DbgWinPlan dbg_win_plan(int64_t k, int64_t w, const DbgHostArrays &H, const int64_t *rcp)
{
    DbgWinPlan P = {};
    P.nref_c = dbg_seq_slots(H.ref_off[w + 1] - H.ref_off[w], k);
    P.read_lo = H.read_lo[w]; P.read_hi = std::max(H.read_lo[w], H.read_hi[w]);
    P.C = dbg_window_occ(k, H.ref_off[w + 1] - H.ref_off[w], rcp, P.read_lo, P.read_hi);
    P.ref_off = H.ref_off[w]; P.ref_pos = H.ref_pos[w];
    P.nc = dbg_node_slots(P.C); P.ec = dbg_edge_slots(P.C);
    return P;
}
inline int64_t dbg_max_occ(int64_t k, const DbgHostArrays &H, const int64_t *rcp)
{
    int64_t m = 0;
    for (int64_t w = 0; w < (int64_t)H.ref_pos.size(); ++w) m = std::max(m, dbg_win_plan(k, w, H, rcp).C);
    return m;
}

// a window's tables: 36 bytes a node slot and an edge slot, 8 an occurrence slot
inline size_t dbg_window_bytes(int64_t C) { return (size_t)(dbg_node_slots(C) * 36 + dbg_edge_slots(C) * 36 + 8 * C); }
// what one window takes of an assembly range: its tables, 2C nodes, C edges, 2C in-degrees, list entries and pointers
inline size_t dbg_asm_window_bytes(int64_t C) { return align256(dbg_window_bytes(C)) + (size_t)C * (2 * sizeof(gbx_dbg_node) + sizeof(gbx_dbg_edge) + 24); }

// The room for windows of which the largest takes `one` bytes and all together `all` (_of: n_win times `one`): everything up to
// DBG_AREA_BYTES, and one window whatever it takes.
inline size_t dbg_area_bytes(size_t one, size_t all) { return std::max(one, std::min(all, DBG_AREA_BYTES)); }
inline size_t dbg_area_bytes_of(size_t one, int64_t n_win)
{
    return dbg_area_bytes(one, n_win > 0 && one > ((size_t)-1) / (size_t)n_win ? (size_t)-1 : one * (size_t)std::max<int64_t>(n_win, 1));
}

// ---- the build (gbx_dbg_build_*, gbx_dbg_graph_*).  The workspace: the reads' slot prefix, the plan, the error word, then the
// batches' table region to the end; bytes: with a region for n_win windows of max_occ slots at most.
struct DbgBuildLayout { size_t rcp, plan, err, region, bytes; };
inline DbgBuildLayout dbg_build_layout(int64_t n_win, int64_t n_reads, int64_t max_occ)
{
    Carver c; DbgBuildLayout L;
    L.rcp = c((size_t)(n_reads + 1) * 8); L.plan = c((size_t)std::max<int64_t>(n_win, 1) * sizeof(DbgWinPlan)); L.err = c(256);
    L.region = c.at; L.bytes = L.region + dbg_area_bytes_of(dbg_window_bytes(max_occ), n_win);
    return L;
}

// Windows [w0, w1) cut into batches whose tables fit table_bytes (and of DBG_BATCH_WINDOWS at most): plan[batches[b] ..
// batches[b + 1]) is batch b, win counts from w0.  Returns -1, or the first window whose tables alone do not fit.
inline int64_t dbg_cut_batches(int64_t k, int64_t w0, int64_t w1, const DbgHostArrays &H, const int64_t *rcp, size_t table_bytes,
                               std::vector<DbgWinPlan> &plan, std::vector<int64_t> &batches)
{
    plan.clear(); batches.assign(1, 0);
    int64_t cand = 0; size_t used = 0;
    for (int64_t w = w0; w < w1; ++w) {
        DbgWinPlan P = dbg_win_plan(k, w, H, rcp);
        const size_t b = dbg_window_bytes(P.C);
        if (b > table_bytes) return w;
        if (used + b > table_bytes || (int64_t)plan.size() - batches.back() >= DBG_BATCH_WINDOWS) {
            batches.push_back((int64_t)plan.size());
            used = 0; cand = 0;
        }
        P.win = w - w0; P.base = (int64_t)used; P.cand0 = cand;
        used += b; cand += P.C;
        plan.push_back(P);
    }
    if (batches.back() != (int64_t)plan.size()) batches.push_back((int64_t)plan.size());
    return -1;
}

// ---- the assembly (gbx_dbg_assemble_*).  A range inside the area: the windows' tables (each at a multiple of 256), then the
// graphs' five arrays; at most, for windows whose dbg_asm_window_bytes sum to window_bytes, a rounding to 256 more per piece.
enum { DBG_ASM_TABLES, DBG_ASM_NODES, DBG_ASM_EDGES, DBG_ASM_DEG, DBG_ASM_LIST, DBG_ASM_NXT, DBG_ASM_PIECES };
struct DbgAsmRangeLayout { size_t at[DBG_ASM_PIECES], bytes; };
inline DbgAsmRangeLayout dbg_asm_range_layout(size_t tables, int64_t node_cap, int64_t edge_cap)
{
    Carver c; DbgAsmRangeLayout L;
    L.at[DBG_ASM_TABLES] = c(tables); L.at[DBG_ASM_NODES] = c((size_t)node_cap * sizeof(gbx_dbg_node)); L.at[DBG_ASM_EDGES] = c((size_t)edge_cap * sizeof(gbx_dbg_edge));
    L.at[DBG_ASM_DEG] = c((size_t)node_cap * 4); L.at[DBG_ASM_LIST] = c((size_t)node_cap * 4); L.at[DBG_ASM_NXT] = c((size_t)node_cap * 4);
    L.bytes = c.at;
    return L;
}
inline size_t dbg_asm_range_bytes(size_t window_bytes) { return window_bytes + (size_t)DBG_ASM_PIECES * 256; }

// The workspace: the head for the call, the searches' path buffer (path_blocks slices of path_slice ints), then the area of the
// ranges to the end.  least: with an area for the largest window alone, the least a run takes; bytes: for n_win such windows;
// what a range may take of a workspace of work_bytes >= least: dbg_area_bytes(least - area, work_bytes - area).
struct DbgAsmLayout { size_t rcp, plan, err, cyc, win_slot, fin, wstart, counters, node_off, edge_off, pathbuf, area, least, bytes; int64_t path_slice, path_blocks; };
inline DbgAsmLayout dbg_asm_layout(int64_t n_win, int64_t n_reads, int64_t max_occ)
{
    const size_t nw = (size_t)std::max<int64_t>(n_win, 1);
    Carver c; DbgAsmLayout L;
    L.rcp = c((size_t)(n_reads + 1) * 8); L.plan = c(nw * sizeof(DbgWinPlan)); L.err = c(256);
    L.cyc = c(nw * 4); L.win_slot = c(nw * 4); L.fin = c(nw * 4); L.wstart = c(nw * 8); L.counters = c(256);
    L.node_off = c((nw + 1) * 8); L.edge_off = c((nw + 1) * 8);
    L.path_slice = (2 * max_occ + 2 + 63) & ~(int64_t)63;
    L.path_blocks = std::max<int64_t>(1, std::min<int64_t>(DBG_ASM_PATH_BLOCKS, (int64_t)(DBG_ASM_PATH_BYTES / ((size_t)L.path_slice * 4))));
    L.pathbuf = c((size_t)L.path_blocks * (size_t)L.path_slice * 4); L.area = c.at;
    const size_t one = dbg_asm_range_bytes(dbg_asm_window_bytes(max_occ));
    L.least = L.area + one; L.bytes = L.area + dbg_area_bytes_of(one, n_win) + 256;
    return L;
}

// One range of the windows S[done ..) still to do at k: as many as fit `limit` bytes of the area (a lone window goes whatever it
// takes: the entry has checked the workspace against the largest) and DBG_BATCH_WINDOWS at most.  win is the window's index in the
// call, base advances by the tables alone; node_off / edge_off give every window 2C nodes and C edges.  Returns the new done.
struct DbgAsmRange { std::vector<DbgWinPlan> plan; std::vector<int64_t> node_off, edge_off; size_t tables; };
inline size_t dbg_asm_cut_range(int64_t k, const std::vector<int64_t> &S, size_t done, const DbgHostArrays &H, const int64_t *rcp, size_t limit, DbgAsmRange &r)
{
    r.plan.clear(); r.node_off.assign(1, 0); r.edge_off.assign(1, 0);
    size_t window_bytes = r.tables = 0;
    int64_t cand = 0;
    for (; done < S.size() && (int64_t)r.plan.size() < DBG_BATCH_WINDOWS; ++done) {
        DbgWinPlan P = dbg_win_plan(k, S[done], H, rcp);
        const size_t b = dbg_asm_window_bytes(P.C);
        if (dbg_asm_range_bytes(window_bytes + b) > limit && !r.plan.empty()) break;
        P.win = S[done]; P.base = (int64_t)r.tables; P.cand0 = cand;
        r.tables += align256(dbg_window_bytes(P.C));
        window_bytes += b; cand += P.C;
        r.node_off.push_back(r.node_off.back() + 2 * P.C);
        r.edge_off.push_back(r.edge_off.back() + P.C);
        r.plan.push_back(P);
    }
    return done;
}

}  // namespace gbx
