// dbg_plan_check.cpp — TEST-ONLY host build of the dbg family's planning rules (genomicsbench_amd/csrc/dbg_plan.h, the header
// capi_dbg.hip and capi_dbg_asm.hip plan with): the two cutters as the entries call them and the two workspace layouts, for
// tests/test_dbg_plan_cpu.py's restatement.  g++ -O2 -std=c++17 -Wall -fPIC -shared; tests/sanitize_dbg_plan builds the same
// functions into a program of its own under ASan + UBSan.
#include "../../genomicsbench_amd/csrc/dbg_plan.h"

using namespace gbx;

static DbgHostArrays arrays(int64_t n_reads, const int64_t *seq_off, int64_t n_win, const int64_t *ref_off, const int64_t *ref_pos, const int64_t *read_lo,
                            const int64_t *read_hi)
{
    DbgHostArrays H;
    H.seq_off.assign(seq_off, seq_off + n_reads + 1);
    H.ref_off.assign(ref_off, ref_off + n_win + 1);
    H.ref_pos.assign(ref_pos, ref_pos + n_win);
    H.read_lo.assign(read_lo, read_lo + n_win);
    H.read_hi.assign(read_hi, read_hi + n_win);
    return H;
}

static void put(int64_t *row, const DbgWinPlan &P)
{
    const int64_t v[11] = {P.cand0, P.C, P.nref_c, P.base, P.nc, P.ec, P.read_lo, P.read_hi, P.ref_off, P.ref_pos, P.win};
    for (int j = 0; j < 11; ++j) row[j] = v[j];
}

extern "C" {

// The build's batches of windows [w0, w1) as dbg_device plans them -> the refused window or -1; plan (null: not wanted): 11
// numbers a planned window in DbgWinPlan's order; batches: room for w1 - w0 + 2.
int64_t hostcheck_dbg_batches(int k, int64_t n_reads, const int64_t *seq_off, int64_t n_win, int64_t w0, int64_t w1, const int64_t *ref_off, const int64_t *ref_pos,
                              const int64_t *read_lo, const int64_t *read_hi, uint64_t table_bytes, int64_t *plan, int64_t *n_plan, int64_t *batches,
                              int64_t *n_batches)
{
    const std::vector<int64_t> rcp = dbg_read_prefix(k, n_reads, seq_off);
    std::vector<DbgWinPlan> P;
    std::vector<int64_t> B;
    const int64_t bad = dbg_cut_batches(k, w0, w1, arrays(n_reads, seq_off, n_win, ref_off, ref_pos, read_lo, read_hi), rcp.data(), (size_t)table_bytes, P, B);
    *n_plan = (int64_t)P.size();
    *n_batches = (int64_t)B.size();
    for (size_t j = 0; j < P.size() && plan; ++j) put(plan + 11 * j, P[j]);
    for (size_t j = 0; j < B.size(); ++j) batches[j] = B[j];
    return bad;
}

// The assembly's ranges of the windows S at k in a workspace of work_bytes, as asm_run cuts them (the layout and the limit
// from the call's k0) -> the ranges, or -2 where asm_run refuses the workspace.  plan: 11 numbers a window; per range its end
// in S, the bytes of its tables and the 7 numbers of its layout (DbgAsmRangeLayout); area: the area's bytes.
int64_t hostcheck_dbg_ranges(int k0, int k, int64_t n_reads, const int64_t *seq_off, int64_t n_win, const int64_t *ref_off, const int64_t *ref_pos,
                             const int64_t *read_lo, const int64_t *read_hi, const int64_t *S, int64_t n_S, uint64_t work_bytes, int64_t *plan,
                             int64_t *range_end, uint64_t *tables, uint64_t *layout, uint64_t *area)
{
    const std::vector<int64_t> rcp0 = dbg_read_prefix(k0, n_reads, seq_off), rcp = dbg_read_prefix(k, n_reads, seq_off);
    const DbgHostArrays H = arrays(n_reads, seq_off, n_win, ref_off, ref_pos, read_lo, read_hi);
    const DbgAsmLayout L = dbg_asm_layout(n_win, n_reads, dbg_max_occ(k0, H, rcp0.data()));
    if (work_bytes < L.least) return -2;
    *area = work_bytes - L.area;
    const size_t limit = dbg_area_bytes(L.least - L.area, (size_t)work_bytes - L.area);
    const std::vector<int64_t> todo(S, S + n_S);
    int64_t n = 0;
    DbgAsmRange r;
    for (size_t done = 0; done < todo.size(); ++n) {
        const size_t from = done;
        done = dbg_asm_cut_range(k, todo, done, H, rcp.data(), limit, r);
        for (size_t j = 0; j < r.plan.size() && plan; ++j) put(plan + 11 * (from + j), r.plan[j]);
        const DbgAsmRangeLayout G = dbg_asm_range_layout(r.tables, r.node_off.back(), r.edge_off.back());
        range_end[n] = (int64_t)done;
        tables[n] = r.tables;
        for (int j = 0; j < DBG_ASM_PIECES; ++j) layout[7 * n + j] = G.at[j];
        layout[7 * n + 6] = G.bytes;
    }
    return n;
}

void hostcheck_dbg_build_layout(int64_t n_win, int64_t n_reads, int64_t max_occ, uint64_t *out)
{
    const DbgBuildLayout L = dbg_build_layout(n_win, n_reads, max_occ);
    const uint64_t v[5] = {L.rcp, L.plan, L.err, L.region, L.bytes};
    for (int j = 0; j < 5; ++j) out[j] = v[j];
}

void hostcheck_dbg_asm_layout(int64_t n_win, int64_t n_reads, int64_t max_occ, uint64_t *out)
{
    const DbgAsmLayout L = dbg_asm_layout(n_win, n_reads, max_occ);
    const uint64_t v[16] = {L.rcp, L.plan, L.err, L.cyc, L.win_slot, L.fin, L.wstart, L.counters, L.node_off, L.edge_off, L.pathbuf, L.area,
                            (uint64_t)L.path_slice, (uint64_t)L.path_blocks, L.least, L.bytes};
    for (int j = 0; j < 16; ++j) out[j] = v[j];
}

int64_t hostcheck_dbg_max_occ(int k, int64_t n_reads, const int64_t *seq_off, int64_t n_win, const int64_t *ref_off, const int64_t *ref_pos,
                              const int64_t *read_lo, const int64_t *read_hi)
{
    const std::vector<int64_t> rcp = dbg_read_prefix(k, n_reads, seq_off);
    return dbg_max_occ(k, arrays(n_reads, seq_off, n_win, ref_off, ref_pos, read_lo, read_hi), rcp.data());
}

}  // extern "C"
