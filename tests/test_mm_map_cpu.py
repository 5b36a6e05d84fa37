"""CPU-side checks for the stage behind the chain scores: the restatement (tests/mm_map_ref.py) on the hand vectors of its rules, the
device's rules compiled for the host (mm_map_rules.h in libgbx_mm_cpu.so) against it on every case, the exported symbols, the
parameter and host-entry refusals (all before a device is touched), the PAF text, the mmpaf driver's command line, and the host
build of the rules under ASan + UBSan in a program of its own (tests/sanitize_mm_map)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from genomicsbench_amd import _native as N
from genomicsbench_amd import mm_map as MM
import mm_map_cases as MK
import mm_map_ref as MR
from mm_map_cases import same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MMPAF = os.path.join(ROOT, "genomicsbench_amd", "bin", "mmpaf")
SAN = os.path.join(ROOT, "tests", "sanitize_mm_map")


def _twin():
    L = C.CDLL(os.path.join(ROOT, "genomicsbench_amd", "libgbx_mm_cpu.so"))
    L.gbx_mm_map_cpu.argtypes = [C.POINTER(MM.MmMapParams), C.c_int64] + [C.c_void_p] * 17
    L.gbx_mm_paf_cpu.restype = C.c_int64
    L.gbx_mm_paf_cpu.argtypes = [C.c_int64] + [C.c_void_p] * 6 + [C.c_int64] + [C.c_void_p] * 4 + [C.c_int64, C.c_void_p]
    L.gbx_mm_map_cpu_read_hash.restype = C.c_uint32
    L.gbx_mm_map_cpu_read_hash.argtypes = [C.c_char_p, C.c_int64, C.c_int32]
    return L


def twin_map(b, **kw):
    """the host build of the device's rules on a batch -> the dict MM.map_host gives"""
    p = MM.make_params(**kw)
    n, na = len(b["off"]) - 1, int(b["off"][-1])
    c = lambda a, dt: np.ascontiguousarray(a, dtype=dt)
    off, ax, ay, f, q, v = c(b["off"], np.int64), c(b["ax"], np.uint64), c(b["ay"], np.uint64), c(b["f"], np.int32), c(b["p"], np.int32), c(b["v"], np.int32)
    so, rep, hs = c(b["seq_off"], np.int64), c(b["rep_len"], np.int32), c(b["hash"], np.uint32)
    chain_off, reg_off = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    m = max(na, 1)
    u, cax, cay, nc, regs, cnt = np.zeros(m, np.uint64), np.zeros(m, np.uint64), np.zeros(m, np.uint64), np.zeros(max(n, 1), np.int32), np.zeros(m, MM.REG_DTYPE), np.zeros(2, np.int64)
    _twin().gbx_mm_map_cpu(C.byref(p), n, *[N.ptr(a) for a in (off, ax, ay, f, q, v, so, rep, hs, chain_off, u, cax, cay, nc, reg_off, regs, cnt)])
    return dict(chain_off=chain_off, u=u[:cnt[0]], cax=cax[:na], cay=cay[:na], n_chained=nc[:n], reg_off=reg_off, regs=regs[:cnt[1]],
                counts=(int(cnt[0]), int(cnt[1])))


HAND = dict(p=[-1, 0, 1, 2, 1, -1], f=[15, 30, 45, 40, 50, 15], v=[15, 30, 45, 45, 50, 15])
HAND_AX = [100, 120, 140, 160, 180, 900]
HAND_AY = [15 << 32 | (100 + 20 * i) for i in range(6)]


@pytest.mark.parametrize("min_sc,min_cnt,want", [(40, 2, [(50, [0, 1, 4])]), (15, 2, [(50, [0, 1, 4])]),
                                                 (15, 1, [(50, [0, 1, 4]), (15, [2]), (15, [5])])])
def test_hand_vector_chains(min_sc, min_cnt, want):
    u, a = MR.chains(HAND["f"], HAND["p"], HAND["v"], HAND_AX, HAND_AY, min_sc, min_cnt)
    assert u == [s << 32 | len(c) for s, c in want]
    assert a == [(HAND_AX[i], HAND_AY[i]) for _, c in want for i in c]
    b = dict(off=[0, 6], ax=HAND_AX, ay=HAND_AY, seq_off=[0, 1000], rep_len=[0], hash=[7], **HAND)
    got = twin_map(b, min_chain_score=min_sc, min_cnt=min_cnt)
    assert got["u"].tolist() == u and got["cax"][:len(a)].tolist() == [x for x, _ in a] and got["n_chained"].tolist() == [len(a)]


def _reg(i, score, cnt, qs, qe, rid=0, rs=0, re=100, **kw):
    g = dict(id=i, parent=-1, score=score, subsc=0, cnt=cnt, rid=rid, rev=0, rs=rs, re=re, qs=qs, qe=qe, mlen=0, blen=0, n_sub=0, mapq=0, hash=0, read=0)
    g["as"] = 0
    g.update(kw)
    return g


def test_hand_vectors_parents_selection_mapq():
    """Regions by hand, in score order.  1: inside 0, more anchors (n_sub), kept by the ratio.  2: inside 0, score 62 of 100: below
    0.8 but within min_diff = 40 of it only when min_diff says so.  3: identical to 0 in all five coordinates: dropped uncounted.
    4: beside 0: a second primary.  5: half over 4, the rest uncovered: 0.5 - 0 is not above mask_level: a primary."""
    mk = lambda: [_reg(0, 100, 8, 0, 1000, re=1000), _reg(1, 90, 9, 100, 900, rs=100, re=900), _reg(2, 62, 5, 200, 800, rs=5000, re=5600),
                  _reg(3, 60, 4, 0, 1000, re=1000), _reg(4, 55, 12, 1000, 1400, rid=1), _reg(5, 50, 4, 1200, 1600, rid=1)]
    regs = mk()
    MR.set_parent(regs, 0.5)
    assert [g["parent"] for g in regs] == [0, 0, 0, 0, 4, 5]
    assert (regs[0]["subsc"], regs[0]["n_sub"]) == (90, 1) and regs[4]["n_sub"] == 0
    kept = MR.select_sub(mk_parented(mk), 0.8, 30, 5)
    assert [g["score"] for g in kept] == [100, 90, 55, 50] and [g["parent"] for g in kept] == [0, 0, 2, 3] and [g["id"] for g in kept] == [0, 1, 2, 3]
    kept = MR.select_sub(mk_parented(mk), 0.8, 40, 5)                    # 62 + 40 >= 100: kept by min_diff alone
    assert [g["score"] for g in kept] == [100, 90, 62, 55, 50] and np.float32(62) < np.float32(100) * np.float32(0.8)
    kept = MR.select_sub(mk_parented(mk), 0.8, 40, 1)                    # best_n = 1: the identical one never counted, 62 comes too late
    assert [g["score"] for g in kept] == [100, 90, 55, 50]
    assert len(MR.select_sub(mk_parented(mk), 0.0, 40, 1)) == 6          # pri_ratio 0: no selection
    MR.set_mapq(kept, 0, 40)
    # region 0: pen_cm = min(0.01f * 100, 0.1f * 8) = 0.8; 0.8 * 40 * (1 - 90 / 100) * log(100) = 14.7; n_sub 1: - (int)(4.343 * log 2 + .499) = 3
    # score 55, 12 anchors: 0.55 * 40 * (1 - 40 / 55) * log(55) = 24.04; score 50, 4 anchors: min(0.5, 0.4) * 40 * 0.2 * log(50) = 12.5
    assert [g["mapq"] for g in kept] == [11, 0, 24, 12]
    MR.set_mapq(kept, 500, 40)                                           # rep_len lowers uniq_ratio to 205 / 705: 5.36 - 3, 6.99, 4.55
    assert [g["mapq"] for g in kept] == [2, 0, 6, 4]


def mk_parented(mk):
    regs = mk()
    MR.set_parent(regs, 0.5)
    return regs


def test_uncovered_length_joins_overlapping_primaries():
    """Two primaries that overlap each other under a third region: the union is counted once"""
    regs = [_reg(0, 100, 5, 0, 600), _reg(1, 90, 5, 500, 1000), _reg(2, 80, 5, 450, 1100)]
    MR.set_parent(regs, 0.5)
    # region 1 over 0: ol 100 of min 500, uncovered 400 of max 600: a primary.  Region 2: covered 450..1000, uncovered 100; over 0:
    # 150 / 600 - 100 / 650 < 0.5; over 1: 500 / 500 - 100 / 650 > 0.5
    assert [g["parent"] for g in regs] == [0, 1, 1] and regs[1]["subsc"] == 80 and regs[1]["n_sub"] == 1


@pytest.mark.parametrize("min_sc,min_cnt", MK.FOREST_PARAMS)
def test_twin_on_the_forests(min_sc, min_cnt):
    b = MK.forest_batch()
    same(twin_map(b, min_chain_score=min_sc, min_cnt=min_cnt), MK.forest_expected(min_sc, min_cnt), b)


def test_forests_cover_their_paths():
    tot = MK.forest_coverage()
    assert tot["dup_peak"] and tot["cut_by_dropped"]
    assert sorted(set(np.diff(MK.forest_batch()["off"]).tolist())) == sorted(set(MK.FOREST_SIZES))


@pytest.mark.parametrize("kw", [dict(), dict(min_diff=0, best_n=1), dict(pri_ratio=0.0), dict(mask_level=0.1, min_chain_score=25, min_cnt=2)],
                         ids=["default", "best1", "noselect", "mask0.1"])
def test_twin_on_the_mapped_reads(kw):
    c = MK.map_case()
    want = c["exp"] if not kw else MK.expected(c["batch"], **kw)
    same(twin_map(c["batch"], **kw), want, c["batch"])


def _names(names):
    arena, off = MM.pack_names(names)
    return (arena if len(arena) else np.zeros(1, np.uint8)), off


def twin_paf(regs, reg_off, qnames, seq_off, rep_len, tnames, tseq_off, text_cap):
    qn, qo = _names(qnames)
    tn, to = _names(tnames)
    c = lambda a, dt: np.ascontiguousarray(a, dtype=dt)
    regs, reg_off, seq_off, tseq_off, rep = c(regs, MM.REG_DTYPE), c(reg_off, np.int64), c(seq_off, np.int64), c(tseq_off, np.int64), c(rep_len, np.int32)
    lines, line_off = np.full(text_cap + 8, 0x5a, np.uint8), np.zeros(len(reg_off), np.int64)
    n = _twin().gbx_mm_paf_cpu(len(reg_off) - 1, N.ptr(regs), N.ptr(reg_off), N.ptr(qn), N.ptr(qo), N.ptr(seq_off), N.ptr(rep), len(to) - 1, N.ptr(tn),
                               N.ptr(to), N.ptr(tseq_off), N.ptr(lines), text_cap, N.ptr(line_off))
    return n, lines, line_off


PAF_TABLE = ("q1\t1000\t10\t990\t+\tchrA\t5000\t110\t1100\t800\t995\t60\ttp:A:P\tcm:i:55\ts1:i:790\ts2:i:45\trl:i:0\n"
             "q1\t1000\t10\t400\t-\tchrB\t70\t0\t70\t300\t391\t0\ttp:A:S\tcm:i:20\ts1:i:280\trl:i:0\n"
             "third/read\t31\t0\t31\t-\tchrA\t5000\t4969\t5000\t15\t31\t3\ttp:A:P\tcm:i:3\ts1:i:40\ts2:i:0\trl:i:12\n")


def test_paf_text_of_a_fixed_table():
    regs = np.zeros(3, MM.REG_DTYPE)
    rows = [dict(id=0, parent=0, score=790, subsc=45, cnt=55, rid=0, rev=0, rs=110, re=1100, qs=10, qe=990, mlen=800, blen=995, mapq=60, read=0),
            dict(id=1, parent=0, score=280, subsc=7, cnt=20, rid=1, rev=1, rs=0, re=70, qs=10, qe=400, mlen=300, blen=391, mapq=0, read=0),
            dict(id=0, parent=0, score=40, subsc=0, cnt=3, rid=0, rev=1, rs=4969, re=5000, qs=0, qe=31, mlen=15, blen=31, mapq=3, read=2)]
    for g, row in zip(regs, rows):
        for k, v in row.items():
            g[k] = v
    args = (regs, [0, 2, 2, 3], ["q1", "empty", "third/read"], [0, 1000, 1000, 1031], [0, 5, 12], ["chrA", "chrB"], [0, 5000, 5070])
    n, lines, line_off = twin_paf(*args, text_cap=1000)
    two = PAF_TABLE.index("third/read")
    assert lines[:n].tobytes().decode() == PAF_TABLE and line_off.tolist() == [0, two, two, len(PAF_TABLE)]
    want = MR.paf({k: regs[k].astype(np.int64) for k in MR.REG_FIELDS}, [0, 2, 2, 3], ["q1", "empty", "third/read"], [1000, 0, 31], ["chrA", "chrB"], [5000, 70],
                  [0, 5, 12])
    assert want == PAF_TABLE
    n2, lines, _ = twin_paf(*args, text_cap=100)                        # a capacity in the middle of a line: the need, nothing behind it
    assert n2 == n and lines[:100].tobytes().decode() == PAF_TABLE[:100] and (lines[100:] == 0x5a).all()


def test_paf_of_the_mapped_reads():
    c = MK.map_case()
    b, e = c["batch"], c["exp"]
    regs = np.zeros(len(e["regs"]["id"]), MM.REG_DTYPE)
    for k in MR.REG_FIELDS:
        regs[k] = e["regs"][k]
    tso = np.concatenate([[0], np.cumsum([len(r) for r in c["refs"]])])
    n, lines, line_off = twin_paf(regs, e["reg_off"], c["qnames"], b["seq_off"], b["rep_len"], c["tnames"], tso, len(c["paf"]))
    assert lines[:n].tobytes().decode() == c["paf"] and c["paf"].count("\n") == len(regs) and "tp:A:S" in c["paf"] and "\t-\t" in c["paf"]
    assert line_off[-1] == n and c["paf"][int(line_off[3]):].startswith("read3\t") and line_off[10] == line_off[11] == line_off[12]


def test_hash_vectors():
    assert MR.x31("") == 0 and MR.x31("a") == 97 and MR.x31("ab") == 97 * 31 + 98 and MR.x31("read12") == 0xc8455237
    k = 11                                                                   # W's first step by hand: key += ~(key << 15)
    assert (k + (~(k << 15) & 0xffffffff)) & 0xffffffff == 0xfffa800a
    assert (MR.wang(0), MR.wang(11), MR.wang(1000)) == (0x4636b9c9, 0xc855c661, 0x66bed880)
    assert MR.read_hash("read12", 1000) == 0xe751ccd6 == 0xc8455237 ^ ((0x66bed880 + 0xc855c661) & 0xffffffff)
    L = _twin()
    for name, qlen in (("read12", 1000), ("", 5), ("x", 0), ("a/long name with spaces", 2 ** 31 - 1)):
        want = MR.read_hash(name, qlen)
        assert MM.read_hash(name, qlen) == want and L.gbx_mm_map_cpu_read_hash(name.encode(), len(name), qlen) == want
    assert MR.read_hash("", 5) == (MR.wang(5) + MR.wang(11)) & 0xffffffff


def test_symbols_exported():
    L = N.lib()
    for name in ("map_default_params", "map_check_params", "map_workspace_bytes", "map_device", "map_host", "paf_workspace_bytes", "paf_device",
                 "paf_host"):
        assert hasattr(L, "gbx_mm_" + name), name
    T = _twin()
    assert hasattr(T, "gbx_mm_map_cpu") and hasattr(T, "gbx_mm_cpu_sketch")


def test_default_params():
    p = MM.make_params()
    assert (p.min_cnt, p.min_chain_score, p.best_n, p.min_diff) == (3, 40, 5, 30)
    assert p.mask_level == np.float32(0.5) and p.pri_ratio == np.float32(0.8)
    MM.check_params(p)
    assert C.sizeof(MM.MmMapParams) == 24 and MM.REG_DTYPE.itemsize == 72


@pytest.mark.parametrize("kw,word", [(dict(min_cnt=0), "min_cnt"), (dict(min_chain_score=-1), "min_chain_score"), (dict(best_n=-1), "best_n"),
                                     (dict(mask_level=float("nan")), "mask_level"), (dict(pri_ratio=float("nan")), "pri_ratio")])
def test_check_params_refuses(kw, word):
    with pytest.raises(N.GbxError) as e:
        MM.check_params(MM.make_params(**kw))
    assert e.value.code == N.GBX_ERR_ARG and word in str(e.value)


def test_host_entries_refuse_before_a_device():
    L, p = MM.lib(), MM.make_params()
    err = lambda: L.gbx_last_error().decode()
    i64 = lambda *v: np.array(v, np.int64)
    ax, f = np.zeros(8, np.uint64), np.zeros(8, np.int32)
    par = np.full(8, -1, np.int32)
    rep, hs, nc, cnt = np.zeros(4, np.int32), np.zeros(4, np.uint32), np.zeros(4, np.int32), np.zeros(2, np.int64)
    co, ro, u, regs = np.zeros(4, np.int64), np.zeros(4, np.int64), np.zeros(8, np.uint64), np.zeros(8, MM.REG_DTYPE)

    def go(n, off, seq_off, par_=par, ax_=ax, co_=co, chain_cap=8, reg_cap=8, p_=p, u_=u):
        return L.gbx_mm_map_host(C.byref(p_), n, N.ptr(off), N.ptr(ax_), N.ptr(ax), N.ptr(f), N.ptr(par_), N.ptr(f), N.ptr(seq_off), N.ptr(rep), N.ptr(hs),
                                 N.ptr(co_), N.ptr(u_), chain_cap, N.ptr(ax), N.ptr(ax), N.ptr(nc), N.ptr(ro), N.ptr(regs), reg_cap, N.ptr(cnt))
    so = i64(0, 100, 200)
    assert go(2, None, so) == N.GBX_ERR_ARG and "null" in err()
    assert go(2, i64(0, 3, 8), None) == N.GBX_ERR_ARG and "null" in err()
    assert go(2, i64(0, 3, 8), so, ax_=None) == N.GBX_ERR_ARG and "null" in err()
    assert go(2, i64(0, 3, 8), so, co_=None) == N.GBX_ERR_ARG and "null" in err()
    assert go(2, i64(0, 3, 8), so, u_=None) == N.GBX_ERR_ARG and "null" in err()
    assert go(2, i64(1, 3, 8), so) == N.GBX_ERR_ARG and "off[0]" in err()
    assert go(2, i64(0, 5, 3), so) == N.GBX_ERR_ARG and "off is not monotone at read 1" in err()
    assert go(2, i64(0, 3, 8), i64(0, 100, 50)) == N.GBX_ERR_ARG and "seq_off is not monotone at read 1" in err()
    assert go(2, i64(0, 3, 3 + 2 ** 31), so) == N.GBX_ERR_UNSUPPORTED and "read 1" in err()
    assert go(2, i64(0, 3, 8), so, chain_cap=-1) == N.GBX_ERR_ARG
    assert go(2, i64(0, 3, 8), so, reg_cap=-1) == N.GBX_ERR_ARG
    assert go(2 ** 21 + 1, i64(0, 3, 8), so) == N.GBX_ERR_UNSUPPORTED and "reads" in err()
    assert go(2, i64(0, 3, 8), so, p_=MM.make_params(min_cnt=0)) == N.GBX_ERR_ARG and "min_cnt" in err()
    bad = par.copy()
    bad[4] = 1                                                               # anchor 1 of read 1 names itself
    assert go(2, i64(0, 3, 8), so, par_=bad) == N.GBX_ERR_ARG and "anchor 1 of read 1" in err()
    bad[4] = -2
    assert go(2, i64(0, 3, 8), so, par_=bad) == N.GBX_ERR_ARG and "parent = -2" in err()
    assert go(0, i64(0), i64(0)) == N.GBX_OK and cnt.tolist() == [0, 0]
    # PAF
    lo, nt = np.zeros(4, np.int64), C.c_int64(0)
    names, noff = np.frombuffer(b"abcd", np.uint8).copy(), i64(0, 2, 4)
    regs["read"][:3] = [0, 1, 1]

    def paf(n, reg_off, qoff=noff, toff=noff, tso=i64(0, 50, 90), lines=ax, text_cap=64, lo_=lo):
        return L.gbx_mm_paf_host(n, N.ptr(regs), N.ptr(reg_off), N.ptr(names), N.ptr(qoff), N.ptr(so), N.ptr(rep), 2, N.ptr(names), N.ptr(toff), N.ptr(tso),
                                 N.ptr(lines), text_cap, N.ptr(lo_), C.byref(nt))
    assert paf(2, None) == N.GBX_ERR_ARG and "null" in err()
    assert paf(2, i64(0, 1, 3), lines=None) == N.GBX_ERR_ARG and "null" in err()
    assert paf(2, i64(0, 1, 3), lo_=None) == N.GBX_ERR_ARG and "null" in err()
    assert paf(2, i64(0, 2, 1)) == N.GBX_ERR_ARG and "reg_off is not monotone at read 1" in err()
    assert paf(2, i64(0, 1, 3), qoff=i64(0, 3, 2)) == N.GBX_ERR_ARG and "qname_off" in err()
    assert paf(2, i64(0, 1, 3), toff=i64(1, 2, 4)) == N.GBX_ERR_ARG and "tname_off[0]" in err()
    assert paf(2, i64(0, 1, 3), tso=i64(0, 50, 40)) == N.GBX_ERR_ARG and "tseq_off is not monotone at target 1" in err()
    assert paf(2, i64(0, 1, 3), text_cap=-1) == N.GBX_ERR_ARG
    assert paf(2, i64(0, 2, 3)) == N.GBX_ERR_ARG and "region 1 names read 1" in err()
    assert paf(0, i64(0)) == N.GBX_OK and nt.value == 0


def test_device_entries_refuse_bad_arguments():
    L, p = MM.lib(), MM.make_params()
    assert L.gbx_mm_map_device(C.byref(p), 1, *([None] * 3), 10, *([None] * 8), 10, *([None] * 5), 10, None, None, 0, None) == N.GBX_ERR_ARG
    assert L.gbx_mm_map_device(C.byref(p), 2 ** 21 + 1, *([None] * 3), 0, *([None] * 8), 0, *([None] * 5), 0, None, None, 0, None) == N.GBX_ERR_UNSUPPORTED
    assert L.gbx_mm_paf_device(1, None, None, None, 4, None, None, None, None, 1, None, None, None, None, 10, None, None, None, 0, None) == N.GBX_ERR_ARG
    assert L.gbx_mm_map_workspace_bytes(4, 1000, 300) >= 1000 * 36 + 300 * (72 + 16 + 4)
    assert L.gbx_mm_map_workspace_bytes(-1, 1000, 300) == 0 and L.gbx_mm_paf_workspace_bytes(4, 100) >= 808


@pytest.mark.parametrize("min_sc,min_cnt", [(40, 3), (15, 1)])
def test_rules_under_asan_ubsan(tmp_path, min_sc, min_cnt):
    """The host build of the rules and of the PAF writer in a stand-alone program under ASan + UBSan (tests/sanitize_mm_map), every
    buffer exactly as large as the entry names, on the forests: clean, and the restatement's chains, regions and text."""
    r = subprocess.run(["make", "-C", SAN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    b, want = MK.forest_batch(), MK.forest_expected(min_sc, min_cnt)
    n, na = len(b["off"]) - 1, int(b["off"][-1])
    src, out = tmp_path / "batch.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.array([n, na], np.int64).tobytes())
        for k, dt in (("off", np.int64), ("seq_off", np.int64), ("ax", np.uint64), ("ay", np.uint64), ("f", np.int32), ("p", np.int32), ("v", np.int32),
                      ("rep_len", np.int32), ("hash", np.uint32)):
            f.write(np.ascontiguousarray(b[k], dtype=dt).tobytes())
    r = subprocess.run([os.path.join(SAN, "_build", "map_main"), str(src), str(out), str(min_sc), str(min_cnt)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    raw = open(out, "rb").read()
    cnt = np.frombuffer(raw, np.int64, 2)
    assert cnt.tolist() == [len(want["u"]), len(want["regs"]["id"])]
    at = 16
    chain_off, reg_off = np.frombuffer(raw, np.int64, n + 1, at), np.frombuffer(raw, np.int64, n + 1, at + 8 * (n + 1))
    at += 16 * (n + 1)
    u = np.frombuffer(raw, np.uint64, cnt[0], at)
    regs = np.frombuffer(raw, MM.REG_DTYPE, cnt[1], at + 8 * cnt[0])
    at += 8 * cnt[0] + 72 * cnt[1]
    assert np.array_equal(chain_off, want["chain_off"]) and np.array_equal(reg_off, want["reg_off"]) and np.array_equal(u, want["u"])
    for k in MR.REG_FIELDS:
        assert np.array_equal(regs[k].astype(np.int64), want["regs"][k]), k
    n_text = int(np.frombuffer(raw, np.int64, 1, at)[0])
    text = MR.paf(want["regs"], want["reg_off"], ["read%d" % i for i in range(n)], b["qlen"], ["ref0", "ref1"], [100000, 100000], b["rep_len"])
    assert raw[at + 8:].decode() == text and n_text == len(text)


def test_mmpaf_command_line(tmp_path):
    run = lambda *a: subprocess.run([MMPAF] + list(a), capture_output=True, text=True, timeout=60)
    r = run("--help")
    assert r.returncode == 0 and r.stdout.startswith("usage: mmpaf") and "--mid-occ" in r.stdout and "-N" in r.stdout
    for args, word in ((("-k",), "-k takes an integer"), (("-n", "x", "a", "b"), "-n takes an integer"), (("-q", "a", "b"), "unknown option -q"),
                       (("a",), "a reference and a read file"), (("-k", "29", "a", "b"), "k = 29"), (("-n", "0", "a", "b"), "min_cnt"),
                       (("-m", "-1", "a", "b"), "min_chain_score"), (("-N", "-2", "a", "b"), "best_n"), (("-M", "z", "a", "b"), "-M takes a number"),
                       (("-p",), "-p takes a number")):
        r = run(*args)
        assert r.returncode == 1 and word in r.stderr, (args, r.stderr)
    fa = tmp_path / "ref.fa"
    fa.write_text(">r\nACGT\n")
    r = run(str(fa), str(tmp_path / "absent.fq"))
    assert r.returncode == 1 and "fail to open" in r.stderr
