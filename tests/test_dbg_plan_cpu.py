"""The host side of the dbg family, on the CPU alone.  csrc/dbg_plan.h - the build's batch cutter, the assembly's range
cutter and the two workspace layouts, built for the host by tests/hostcheck/dbg_plan_check.cpp - against a literal
restatement of the rules as the entries had them inline before they moved there; the two sizing entries against the sizes
recorded before the move (tests/golden/dbg_workspace_sizes.json); the host entries' refusals, which all come before the
first device call, with their codes and texts; and the planner in a program of its own under ASan + UBSan
(tests/sanitize_dbg_plan)."""
import copy
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import dbg_asm_cases as AC
from genomicsbench_amd import _native as N
from genomicsbench_amd import dbg as D
from genomicsbench_amd import dbg_asm as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "tests", "sanitize_dbg_plan")
I64P, U64P = C.POINTER(C.c_int64), C.POINTER(C.c_uint64)


@pytest.fixture(scope="module")
def hostcheck():
    src = os.path.join(ROOT, "tests", "hostcheck", "dbg_plan_check.cpp")
    out = os.path.join(ROOT, "tests", "hostcheck", "libdbg_plan_check.so")
    hdrs = [os.path.join(ROOT, "genomicsbench_amd", "csrc", h) for h in ("dbg_plan.h", "dbg_hash.h", "carver.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in [src] + hdrs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", src, "-o", out], check=True)
    L = C.CDLL(out)
    i64, u64, vp = C.c_int64, C.c_uint64, C.c_void_p
    L.hostcheck_dbg_batches.argtypes = [C.c_int, i64, vp, i64, i64, i64, vp, vp, vp, vp, u64, vp, I64P, vp, I64P]
    L.hostcheck_dbg_batches.restype = i64
    L.hostcheck_dbg_ranges.argtypes = [C.c_int, C.c_int, i64, vp, i64, vp, vp, vp, vp, vp, i64, u64, vp, vp, vp, vp, U64P]
    L.hostcheck_dbg_ranges.restype = i64
    L.hostcheck_dbg_build_layout.argtypes = [i64, i64, i64, vp]
    L.hostcheck_dbg_asm_layout.argtypes = [i64, i64, i64, vp]
    L.hostcheck_dbg_max_occ.argtypes = [C.c_int, i64, vp, i64, vp, vp, vp, vp]
    L.hostcheck_dbg_max_occ.restype = i64
    return L


# ------------------------------------------------------------------------------------------------ the restatement
# The rules as the entries had them before csrc/dbg_plan.h: the build's dbg_plan(), the assembly's range loop with its head,
# path buffer and slack, and the two sizing entries.
TABLE_BYTES = RANGE_BYTES = 2 << 30
RANGE_SLACK = 6 * 256
PLAN_BYTES = 88                                   # sizeof(DbgWinPlan): eleven int64
_sizes = {}


def a256(v):
    return (v + 255) & ~255


def sizes(c):
    if c not in _sizes:
        nc = ec = 2
        while nc < 2 * c + 1:
            nc <<= 1
        while ec < c + 1:
            ec <<= 1
        _sizes[c] = (nc, ec)
    return _sizes[c]


def window_bytes(c):
    nc, ec = sizes(c)
    return nc * 36 + ec * 36 + 8 * c


def asm_window_bytes(c):
    return a256(window_bytes(c)) + c * (2 * 32 + 16 + 24)


def prefix(k, seq_off):
    rcp = [0]
    for r in range(len(seq_off) - 1):
        rcp.append(rcp[-1] + max(0, seq_off[r + 1] - seq_off[r] - k - 1))
    return rcp


def one_all_cap(one, n_win, cap):
    return max(one, min(one * max(n_win, 1), cap))


def build_head(n_win, n_reads):
    return a256((n_reads + 1) * 8) + a256(max(n_win, 1) * PLAN_BYTES) + 256


def build_workspace(n_win, n_reads, occ):
    return build_head(n_win, n_reads) + one_all_cap(window_bytes(occ), n_win, TABLE_BYTES)


def asm_head_pieces(n_win, n_reads):
    nw = max(n_win, 1)
    return [(n_reads + 1) * 8, nw * PLAN_BYTES, 256, nw * 4, nw * 4, nw * 4, nw * 8, 256, (nw + 1) * 8, (nw + 1) * 8]


def asm_paths(occ):
    slice_ = (2 * occ + 2 + 63) & ~63
    blocks = max(1, min(1024, (256 << 20) // (slice_ * 4)))
    return slice_, blocks, a256(blocks * slice_ * 4)


def asm_workspace(n_win, n_reads, occ):
    head = sum(a256(b) for b in asm_head_pieces(n_win, n_reads))
    return head + asm_paths(occ)[2] + one_all_cap(asm_window_bytes(occ) + RANGE_SLACK, n_win, RANGE_BYTES) + 256


def parent_batches(k, w0, w1, call, table_bytes):
    """-> (refused window or -1, plan rows, batches)"""
    roff, rpos, rlo, rhi = call["ref_off"], call["ref_pos"], call["read_lo"], call["read_hi"]
    rcp = prefix(k, call["seq_off"])
    plan, batches, cand, used = [], [0], 0, 0
    for w in range(w0, w1):
        nref = max(0, roff[w + 1] - roff[w] - k - 1)
        lo, hi = rlo[w], max(rlo[w], rhi[w])
        c = nref + rcp[hi] - rcp[lo]
        nc, ec = sizes(c)
        b = window_bytes(c)
        if b > table_bytes:
            return w, plan, batches
        if used + b > table_bytes or len(plan) - batches[-1] >= 1 << 20:
            batches.append(len(plan))
            used = cand = 0
        plan.append((cand, c, nref, used, nc, ec, lo, hi, roff[w], rpos[w], w - w0))
        used += b
        cand += c
    if batches[-1] != len(plan):
        batches.append(len(plan))
    return -1, plan, batches


def max_occ(k, call):
    rcp = prefix(k, call["seq_off"])
    roff, rlo, rhi = call["ref_off"], call["read_lo"], call["read_hi"]
    return max([0] + [max(0, roff[w + 1] - roff[w] - k - 1) + rcp[rhi[w]] - rcp[rlo[w]] for w in range(len(rlo))])


def parent_ranges(k0, k, call, todo, work_bytes):
    """-> None where the entry refuses the workspace, or (plan rows, [(end in todo, table bytes, layout)], area bytes)"""
    roff, rpos, rlo, rhi = call["ref_off"], call["ref_pos"], call["read_lo"], call["read_hi"]
    n_win, n_reads = len(rpos), len(call["seq_off"]) - 1
    occ = max_occ(k0, call)
    head, paths = sum(a256(b) for b in asm_head_pieces(n_win, n_reads)), asm_paths(occ)[2]
    if work_bytes < head + paths + asm_window_bytes(occ) + RANGE_SLACK:
        return None
    area_bytes = work_bytes - head - paths
    limit = min(area_bytes, max(RANGE_BYTES, asm_window_bytes(occ) + RANGE_SLACK))
    rcp = prefix(k, call["seq_off"])
    rows, ranges, done = [], [], 0
    while done < len(todo):
        m = tables = cand = ncap = ecap = 0
        used = RANGE_SLACK
        while done < len(todo) and m < 1 << 20:
            w = todo[done]
            nref = max(0, roff[w + 1] - roff[w] - k - 1)
            lo, hi = rlo[w], max(rlo[w], rhi[w])
            c = nref + rcp[hi] - rcp[lo]
            b = asm_window_bytes(c)
            if used + b > limit and m:
                break
            rows.append((cand, c, nref, tables, sizes(c)[0], sizes(c)[1], lo, hi, roff[w], rpos[w], w))
            tables += a256(window_bytes(c))
            used += b
            cand += c
            ncap += 2 * c
            ecap += c
            m += 1
            done += 1
        q = a256(tables)
        at = [0, q]
        for b in (ncap * 32, ecap * 16, ncap * 4, ncap * 4, ncap * 4):
            q += a256(b)
            at.append(q)
        ranges.append((done, tables, at))
    return rows, ranges, area_bytes


# ------------------------------------------------------------------------------------------------ the calls
def make_call(seed, n_win, n_reads, max_ref=600, empties=()):
    rng = np.random.default_rng(seed)
    seq_off = np.concatenate([[int(rng.integers(0, 9))], rng.integers(0, 152, n_reads)]).cumsum()
    ref_len = rng.integers(0, max_ref + 1, n_win)
    lo = rng.integers(0, n_reads + 1, n_win)
    hi = np.array([int(rng.integers(a, min(n_reads, a + 40) + 1)) for a in lo], dtype=np.int64)
    for w in empties:
        ref_len[w], hi[w] = int(rng.integers(0, 5)), lo[w]
    ref_off = np.concatenate([[int(rng.integers(0, 9))], ref_len]).cumsum()
    return dict(seq_off=[int(x) for x in seq_off], ref_off=[int(x) for x in ref_off], ref_pos=[int(x) for x in rng.integers(0, 1 << 30, n_win)],
                read_lo=[int(x) for x in lo], read_hi=[int(x) for x in hi])


def zero_slot_windows(n):
    return dict(seq_off=[0], ref_off=[0] * (n + 1), ref_pos=[0] * n, read_lo=[0] * n, read_hi=[0] * n)


def calls():
    """(name, k, call): seeded random window lists and the edges"""
    out = [("random_%d" % s, (3, 15, 31, 64)[s % 4], make_call(s, 5 + 37 * s, 200 + 50 * s)) for s in range(8)]
    out.append(("no_windows", 15, make_call(20, 0, 10)))
    out.append(("no_reads", 15, make_call(21, 6, 0)))
    out.append(("one_window", 15, make_call(22, 1, 30)))
    out.append(("empty_first", 15, make_call(23, 9, 100, empties=(0,))))
    out.append(("empty_last", 15, make_call(24, 9, 100, empties=(8,))))
    out.append(("empty_row", 15, make_call(25, 12, 100, empties=(0, 1, 4, 5, 6, 10, 11))))
    out.append(("all_empty", 15, make_call(26, 5, 100, empties=range(5))))
    return out


def arr(x):
    return np.ascontiguousarray(x, dtype=np.int64)


def run_batches(L, k, w0, w1, call, table_bytes, want_plan=True):
    n = max(w1 - w0, 1)
    a = {f: arr(v) for f, v in call.items()}
    plan, batches = np.zeros((n, 11), dtype=np.int64), np.zeros(n + 2, dtype=np.int64)
    n_plan, n_batches = C.c_int64(), C.c_int64()
    bad = L.hostcheck_dbg_batches(k, len(call["seq_off"]) - 1, N.ptr(a["seq_off"]), len(call["ref_pos"]), w0, w1, N.ptr(a["ref_off"]), N.ptr(a["ref_pos"]), N.ptr(a["read_lo"]),
                                  N.ptr(a["read_hi"]), table_bytes, N.ptr(plan) if want_plan else None, C.byref(n_plan), N.ptr(batches), C.byref(n_batches))
    return bad, plan[:n_plan.value], [int(x) for x in batches[:n_batches.value]]


def run_ranges(L, k0, k, call, todo, work_bytes, want_plan=True):
    n = max(len(todo), 1)
    a = {f: arr(v) for f, v in call.items()}
    s = arr(todo)
    plan, end = np.zeros((n, 11), dtype=np.int64), np.zeros(n, dtype=np.int64)
    tables, layout, area = np.zeros(n, dtype=np.uint64), np.zeros((n, 7), dtype=np.uint64), C.c_uint64()
    got = L.hostcheck_dbg_ranges(k0, k, len(call["seq_off"]) - 1, N.ptr(a["seq_off"]), len(call["ref_pos"]), N.ptr(a["ref_off"]), N.ptr(a["ref_pos"]),
                                 N.ptr(a["read_lo"]), N.ptr(a["read_hi"]), N.ptr(s), len(todo), work_bytes, N.ptr(plan) if want_plan else None, N.ptr(end),
                                 N.ptr(tables), N.ptr(layout), C.byref(area))
    if got < 0:
        return None
    return plan[:len(todo)], [(int(end[j]), int(tables[j]), [int(x) for x in layout[j]]) for j in range(got)], int(area.value)


def build_layout(L, n_win, n_reads, occ):
    out = np.zeros(5, dtype=np.uint64)
    L.hostcheck_dbg_build_layout(n_win, n_reads, occ, N.ptr(out))
    return [int(x) for x in out]


def asm_layout(L, n_win, n_reads, occ):
    out = np.zeros(16, dtype=np.uint64)
    L.hostcheck_dbg_asm_layout(n_win, n_reads, occ, N.ptr(out))
    return [int(x) for x in out]


def same_batches(L, k, w0, w1, call, table_bytes, what):
    bad, plan, batches = run_batches(L, k, w0, w1, call, table_bytes)
    want = parent_batches(k, w0, w1, call, table_bytes)
    assert (bad, batches) == (want[0], want[2]), what
    assert [tuple(int(x) for x in r) for r in plan] == want[1], what
    return want


def same_ranges(L, k0, k, call, todo, work_bytes, what):
    got, want = run_ranges(L, k0, k, call, todo, work_bytes), parent_ranges(k0, k, call, todo, work_bytes)
    assert (got is None) == (want is None), what
    if want is None:
        return None
    assert [tuple(int(x) for x in r) for r in got[0]] == want[0], what
    assert got[2] == want[2] and [(e, t, at) for e, t, at in got[1]] == want[1], what
    assert all(at[-1] <= got[2] for _, _, at in got[1]), "%s: a range's layout ends outside the area" % what
    return want


# ------------------------------------------------------------------------------------------------ the tests
def test_sizes_are_the_recorded_ones():
    """both sizing entries, byte for byte, over the whole grid recorded before the layouts moved"""
    with open(os.path.join(ROOT, "tests", "golden", "dbg_workspace_sizes.json")) as f:
        rows = json.load(f)["rows"]
    assert len(rows) == 6 * 4 * 7
    p = D.make_params()
    for nw, nr, occ, build, asm in rows:
        assert N.lib().gbx_dbg_workspace_bytes(C.byref(p), nw, nr, occ) == build, (nw, nr, occ)
        assert N.lib().gbx_dbg_assemble_workspace_bytes(C.byref(p), nw, nr, occ) == asm, (nw, nr, occ)
        assert (build_workspace(nw, nr, occ), asm_workspace(nw, nr, occ)) == (build, asm), (nw, nr, occ)


def test_layouts_equal_the_restatement(hostcheck):
    for nw in (0, 1, 2, 7, 4096, 16000):
        for nr in (0, 1, 1000, 3200000):
            for occ in (0, 1, 63, 64, 150000, 1 << 24):
                got = build_layout(hostcheck, nw, nr, occ)
                assert got == [0, a256((nr + 1) * 8), build_head(nw, nr) - 256, build_head(nw, nr), build_workspace(nw, nr, occ)]
                got = asm_layout(hostcheck, nw, nr, occ)
                at = [0]
                for b in asm_head_pieces(nw, nr) + [asm_paths(occ)[2]]:
                    at.append(at[-1] + a256(b))
                assert got[:12] == at and got[12:14] == list(asm_paths(occ)[:2])
                assert got[14:] == [at[-1] + asm_window_bytes(occ) + RANGE_SLACK, asm_workspace(nw, nr, occ)]


@pytest.mark.parametrize("name,k,call", calls(), ids=[c[0] for c in calls()])
def test_batches_equal_the_restatement(hostcheck, name, k, call):
    """the same batches, base and cand0 at table sizes from the largest window alone to all windows, sub-ranges with w0 > 0,
    and the same refusal below the largest window"""
    n = len(call["ref_pos"])
    rcp = prefix(k, call["seq_off"])
    b = [window_bytes(max(0, call["ref_off"][w + 1] - call["ref_off"][w] - k - 1) + rcp[call["read_hi"][w]] - rcp[call["read_lo"][w]]) for w in range(n)]
    big, total = max(b + [0]), sum(b)
    for table in sorted(t for t in {big, big + 1, big + 143, 2 * big, (big + total) // 2, total - 1, total, total + 1} if t >= big):
        want = same_batches(hostcheck, k, 0, n, call, table, (name, table))
        assert want[0] == -1 and (table < total or len(want[2]) <= 2)
    for w0, w1 in ((1, n), (n // 2, n // 2), (n // 3, n - 1)):
        if 0 <= w0 <= w1 <= n:
            same_batches(hostcheck, k, w0, w1, call, big, (name, w0, w1))
    if big > 144:                                 # 144: what a window without slots takes
        for table in (big - 1, big // 2, 144, 0):
            want = same_batches(hostcheck, k, 0, n, call, table, (name, table))
            assert want[0] == min(w for w in range(n) if b[w] > table)


def test_a_window_at_under_and_over_the_table(hostcheck):
    call = make_call(40, 7, 120)
    k, w = 15, 3
    rcp = prefix(k, call["seq_off"])
    b = window_bytes(max(0, call["ref_off"][w + 1] - call["ref_off"][w] - k - 1) + rcp[call["read_hi"][w]] - rcp[call["read_lo"][w]])
    assert b > 144
    assert same_batches(hostcheck, k, w, w + 1, call, b, "at")[0] == -1
    assert same_batches(hostcheck, k, w, w + 1, call, b + 1, "one byte under")[0] == -1
    assert same_batches(hostcheck, k, w, w + 1, call, b - 1, "one byte over")[0] == w


@pytest.mark.parametrize("n", [1 << 20, (1 << 20) + 1])
def test_the_window_cap_of_a_batch_and_a_range(hostcheck, n):
    call = zero_slot_windows(n)
    bad, _, batches = run_batches(hostcheck, 15, 0, n, call, 1 << 30, want_plan=False)
    want = parent_batches(15, 0, n, call, 1 << 30)
    assert (bad, batches) == (-1, want[2]) and batches == ([0, n] if n == 1 << 20 else [0, 1 << 20, n])
    work = asm_workspace(n, 0, 0)
    got, want = run_ranges(hostcheck, 15, 15, call, range(n), work, want_plan=False), parent_ranges(15, 15, call, range(n), work)
    assert got[1] == want[1] and got[2] == want[2] and [e for e, _, _ in got[1]] == ([n] if n == 1 << 20 else [1 << 20, n])


@pytest.mark.parametrize("name,k,call", calls(), ids=[c[0] for c in calls()])
def test_ranges_equal_the_restatement(hostcheck, name, k, call):
    """the same ranges, base, cand0 and layouts with the area at the sizing entry's least, at its full size and between, in
    the first round and in a later one (larger k, a subset of the windows); never a refusal in a workspace of the sizing
    entry's, whole or by test_dbg_asm_gpu.py's small recipe; one a byte below the least"""
    n, nr = len(call["ref_pos"]), len(call["seq_off"]) - 1
    occ = max_occ(k, call)
    assert occ == hostcheck.hostcheck_dbg_max_occ(k, nr, N.ptr(arr(call["seq_off"])), n, N.ptr(arr(call["ref_off"])), N.ptr(arr(call["ref_pos"])), N.ptr(arr(call["read_lo"])),
                                                  N.ptr(arr(call["read_hi"])))
    lay = asm_layout(hostcheck, n, nr, occ)
    least, full = lay[14], lay[15]
    small = asm_workspace(1, 0, occ) + asm_workspace(n, nr, 0) - asm_workspace(1, 0, 0)
    later = [w for w in range(n) if w % 3 != 1]
    for work in sorted({least, least + 1, small, (least + full) // 2, full}):
        assert same_ranges(hostcheck, k, k, call, list(range(n)), work, (name, work)) is not None
        assert same_ranges(hostcheck, k, min(64, k + 5), call, later, work, (name, work, "later")) is not None
    assert same_ranges(hostcheck, k, k, call, list(range(n)), least - 1, (name, "below")) is None


def test_planner_under_asan_ubsan():
    """csrc/dbg_plan.h in a stand-alone program under ASan + UBSan: both cutters and both layouts over seeded random window
    lists and the edges above, every plan inside its tables and every range inside its area"""
    r = subprocess.run(["make", "-C", SAN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([os.path.join(SAN, "_build", "dbg_plan_main")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    words = r.stdout.split()
    assert words[0] == "ok" and int(words[2]) > 1000 and int(words[4]) > 1000, r.stdout


# ------------------------------------------------------------------------------------------------ the host entries' refusals
def host_entries(rs_c, ws_c, p, out_caps=(4, 4, 64)):
    """the three host entries on the structs -> [(name, code, text)]"""
    L = N.lib()
    n_win = int(ws_c.n_win) if ws_c is not None and ws_c.n_win > 0 else 0
    nw = max(n_win, 1)
    st = np.zeros(nw, dtype=D.STATS_DTYPE)
    off = np.zeros(nw + 1, dtype=np.int64)
    nodes, edges = np.zeros(1, dtype=D.NODE_DTYPE), np.zeros(1, dtype=D.EDGE_DTYPE)
    wn, starts, paths = np.zeros(nw, dtype=A.WIN_DTYPE), np.zeros(out_caps[0], dtype=A.START_DTYPE), np.zeros(out_caps[1], dtype=A.PATH_DTYPE)
    pn, ps, tot = np.zeros(out_caps[2], dtype=np.int32), np.zeros(out_caps[2], dtype=np.uint8), np.zeros(3, dtype=np.int64)
    o = A.AsmOutC(N.ptr(st), N.ptr(wn), N.ptr(starts), N.ptr(paths), N.ptr(pn), N.ptr(ps), *out_caps, N.ptr(tot))
    ap = A.make_asm_params()
    r = C.byref(rs_c) if rs_c is not None else None
    w = C.byref(ws_c) if ws_c is not None else None
    out = []
    for name, call in (("gbx_dbg_build_host", lambda: L.gbx_dbg_build_host(C.byref(p), r, w, N.ptr(st))),
                       ("gbx_dbg_graph_host", lambda: L.gbx_dbg_graph_host(C.byref(p), r, w, 0, n_win, N.ptr(off), N.ptr(off), N.ptr(nodes), N.ptr(edges))),
                       ("gbx_dbg_assemble_host", lambda: L.gbx_dbg_assemble_host(C.byref(p), C.byref(ap), r, w, C.byref(o)))):
        code = call()
        out.append((name, code, L.gbx_last_error().decode()))
    return out


def spoiled():
    """[(what, reads struct, windows struct, code, the text behind "<entry>: ")], what keeps their arrays alive, the good call"""
    case = {c.name: c for c in AC.all_cases()}["starts_of_several_windows"]
    rs, ws, _ = case.packed()
    n, nw = rs.n_reads, ws.n_win
    assert n >= 2 and nw >= 2
    keep, out = [], []

    def add(what, code, text, reads=None, wins=None, r_set=(), w_set=()):
        r2, w2 = copy.deepcopy(rs), copy.deepcopy(ws)
        for f, i, v in reads or ():
            getattr(r2, f)[i] = v
        for f, i, v in wins or ():
            getattr(w2, f)[i] = v
        keep.extend([r2, w2])
        rc_, wc_ = r2.c_struct(), w2.c_struct()
        for f, v in r_set:
            setattr(rc_, f, v)
        for f, v in w_set:
            setattr(wc_, f, v)
        out.append((what, rc_, wc_, code, text))

    ARG, UNS = N.GBX_ERR_ARG, N.GBX_ERR_UNSUPPORTED
    sizes_text = "n_reads %d, seq_bytes %d, n_win %d, ref_bytes %d"
    add("negative n_reads", ARG, sizes_text % (-1, rs.seq.size, nw, ws.ref.size), r_set=[("n_reads", -1)])
    add("negative seq_bytes", ARG, sizes_text % (n, -1, nw, ws.ref.size), r_set=[("seq_bytes", -1)])
    add("negative n_win", ARG, sizes_text % (n, rs.seq.size, -1, ws.ref.size), w_set=[("n_win", -1)])
    add("negative ref_bytes", ARG, sizes_text % (n, rs.seq.size, nw, -1), w_set=[("ref_bytes", -1)])
    for f in ("seq_off", "seq", "qual", "flag"):
        add("null " + f, ARG, "null read arrays", r_set=[(f, None)])
    for f in ("ref_off", "ref", "ref_pos", "read_lo", "read_hi"):
        add("null " + f, ARG, "null window arrays", w_set=[(f, None)])
    add("seq_off below 0", ARG, "seq_off outside [0, seq_bytes]", reads=[("seq_off", 0, -1)])
    add("seq_off past seq_bytes", ARG, "seq_off outside [0, seq_bytes]", reads=[("seq_off", n, rs.seq.size + 1)])
    add("seq_off decreases", ARG, "seq_off decreases at read 0", reads=[("seq_off", 0, int(rs.seq_off[1]) + 1)])
    add("ref_off below 0", ARG, "ref_off outside [0, ref_bytes]", wins=[("ref_off", 0, -1)])
    add("ref_off past ref_bytes", ARG, "ref_off outside [0, ref_bytes]", wins=[("ref_off", nw, ws.ref.size + 1)])
    add("ref_off decreases", ARG, "window 0: ref_off decreases", wins=[("ref_off", 0, int(ws.ref_off[1]) + 1)])
    add("read_lo > read_hi", ARG, "window 1: its reads are not 0 <= read_lo <= read_hi <= n_reads", wins=[("read_lo", 1, 1), ("read_hi", 1, 0)])
    add("read_lo below 0", ARG, "window 0: its reads are not 0 <= read_lo <= read_hi <= n_reads", wins=[("read_lo", 0, -1)])
    add("read_hi past n_reads", ARG, "window %d: its reads are not 0 <= read_lo <= read_hi <= n_reads" % (nw - 1), wins=[("read_hi", nw - 1, n + 1)])
    add("a reference past 2^31", ARG, "window 1: its reference lies outside [0, 2^31)", wins=[("ref_pos", 1, (1 << 31) - int(ws.ref_off[2] - ws.ref_off[1]))])
    add("a reference below 0", ARG, "window 0: its reference lies outside [0, 2^31)", wins=[("ref_pos", 0, -1)])
    add("2^40 bytes", UNS, "more than 2^40 bytes of reference and reads", r_set=[("seq_bytes", (1 << 40) - ws.ref.size)])
    return out, keep, rs, ws


def test_host_refusals():
    """everything the shared checks refuse returns before the first device call: the code and the text of each, from all
    three host entries"""
    p = D.make_params(3)
    cases, keep, rs, ws = spoiled()
    for name, code, text in host_entries(None, ws.c_struct(), p) + host_entries(rs.c_struct(), None, p):
        assert (code, text) == (N.GBX_ERR_ARG, name + ": null reads or windows")
    for what, r, w, code, want in cases:
        for name, got, text in host_entries(r, w, p):
            assert (got, text) == (code, "%s: %s" % (name, want)), what
