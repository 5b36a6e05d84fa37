"""The stage behind the chain scores on the GPU (gbx_mm_map_*, gbx_mm_paf_*), compared exactly - every integer field, mapq
included, every order and count - with the restatement tests/mm_map_ref.py; the capacities; then reads -> PAF on one stream
(DeviceMmMapper) against the restatement of everything, and the mmpaf driver."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from genomicsbench_amd import _native as N
from genomicsbench_amd import mm_map as MM
from genomicsbench_amd import mm_seed as MS
import mm_map_cases as MK
import mm_map_ref as MR
from mm_map_cases import same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "genomicsbench_amd", "bin")
GUARD = 0x5a5a5a5a5a5a5a5a
GUARD_ROOM = 16


def dev():
    import torch
    return torch.device("cuda:0")


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def device_map(b, p, chain_cap=None, reg_cap=None):
    """gbx_mm_map_device on a batch, the outputs in front of guard words -> dict as MM.map_host gives (cut to the capacities),
    plus `intact`: nothing behind a capacity was touched"""
    import torch
    d = dev()
    n, na = len(b["off"]) - 1, int(b["off"][-1])
    chain_cap = max(na, 1) if chain_cap is None else chain_cap
    reg_cap = max(na, 1) if reg_cap is None else reg_cap
    c = lambda a, dt: np.ascontiguousarray(a, dtype=dt)
    pad = lambda a: a if len(a) else np.zeros(1, a.dtype)
    t = lambda a, dt, view=None: torch.from_numpy(pad(c(a, dt)).view(view or dt)).to(d)
    off, so = t(b["off"], np.int64), t(b["seq_off"], np.int64)
    ax, ay = t(b["ax"], np.uint64, np.int64), t(b["ay"], np.uint64, np.int64)
    f, q, v = t(b["f"], np.int32), t(b["p"], np.int32), t(b["v"], np.int32)
    rep, hs = t(b["rep_len"], np.int32), t(b["hash"], np.uint32, np.int32)
    g = lambda words: torch.from_numpy(np.full(words + GUARD_ROOM, GUARD, np.uint64).view(np.int64)).to(d)
    u, regs, cax, cay = g(chain_cap), g(reg_cap * 9), g(na), g(na)
    chain_off, reg_off = (torch.full((n + 1,), -7, dtype=torch.int64, device=d) for _ in range(2))
    nc, cnt = torch.zeros(max(n, 1), dtype=torch.int32, device=d), torch.full((2,), -7, dtype=torch.int64, device=d)
    L = MM.lib()
    wb = L.gbx_mm_map_workspace_bytes(n, na, chain_cap)
    work = torch.empty(wb, dtype=torch.uint8, device=d)
    N.check(L.gbx_mm_map_device(C.byref(p), n, off.data_ptr(), ax.data_ptr(), ay.data_ptr(), na, f.data_ptr(), q.data_ptr(), v.data_ptr(), so.data_ptr(),
                                rep.data_ptr(), hs.data_ptr(), chain_off.data_ptr(), u.data_ptr(), chain_cap, cax.data_ptr(), cay.data_ptr(), nc.data_ptr(),
                                reg_off.data_ptr(), regs.data_ptr(), reg_cap, cnt.data_ptr(), work.data_ptr(), wb, stream()))
    torch.cuda.synchronize()
    w = lambda x: x.cpu().numpy().view(np.uint64)
    counts = tuple(int(x) for x in cnt.cpu().numpy())
    intact = all((w(x)[cap:] == GUARD).all() for x, cap in ((u, chain_cap), (regs, reg_cap * 9), (cax, na), (cay, na)))
    nu, nr = min(max(counts[0], 0), chain_cap), min(max(counts[1], 0), reg_cap)
    return dict(chain_off=chain_off.cpu().numpy(), u=w(u)[:nu], cax=w(cax)[:na], cay=w(cay)[:na], n_chained=nc.cpu().numpy()[:n],
                reg_off=reg_off.cpu().numpy(), regs=w(regs)[:nr * 9].view(MM.REG_DTYPE), counts=counts, intact=intact,
                keep=(regs, reg_off, cnt, so, rep))


def host_map(b, p, **caps):
    return MM.map_host(p, b["off"], b["ax"], b["ay"], b["f"], b["p"], b["v"], b["seq_off"], b["rep_len"], b["hash"], **caps)


@pytest.mark.parametrize("min_sc,min_cnt", MK.FOREST_PARAMS)
def test_map_device_on_the_forests(min_sc, min_cnt):
    """Reads of 0 .. 5 000 anchors in one call: duplicate peaks, peaks inside earlier walks, walks stopped at marks (kept and dropped),
    peak searches off the root, reads without ends, chains that min_cnt drops and whose marks cut a later one (mm_map_cases asserts them)."""
    MK.forest_coverage()
    b, want = MK.forest_batch(), MK.forest_expected(min_sc, min_cnt)
    got = device_map(b, MM.make_params(min_chain_score=min_sc, min_cnt=min_cnt))
    assert got["intact"] and got["counts"] == (len(want["u"]), len(want["regs"]["id"]))
    same(got, want, b)


@pytest.mark.parametrize("min_sc,min_cnt", MK.FOREST_PARAMS)
def test_map_host_on_the_forests(min_sc, min_cnt):
    b, want = MK.forest_batch(), MK.forest_expected(min_sc, min_cnt)
    same(host_map(b, MM.make_params(min_chain_score=min_sc, min_cnt=min_cnt)), want, b)


VARIANTS = [dict(), dict(min_diff=0, best_n=1), dict(pri_ratio=0.0), dict(mask_level=0.1, min_chain_score=25, min_cnt=2)]


@pytest.mark.parametrize("kw", VARIANTS, ids=["default", "best1", "noselect", "mask0.1"])
def test_map_device_and_host_on_the_mapped_reads(kw):
    """Seeded reads chained by the chain oracle: a reverse-strand region, a secondary, two primaries in a read, rep_len, reads without
    regions (mm_map_cases asserts them)"""
    c = MK.map_case()
    b = c["batch"]
    want = c["exp"] if not kw else MK.expected(b, **kw)
    got = device_map(b, MM.make_params(**kw))
    assert got["intact"]
    same(got, want, b)
    same(host_map(b, MM.make_params(**kw)), want, b)


@pytest.mark.parametrize("short", [0, 1, 200])
def test_chain_capacity(short):
    """chain_cap at, one below and far below the need: the count is the need, chain_off stays true, u is the head of the list, nothing
    behind the capacity is touched; without room for all chains no regions are made (-1, reg_off all 0)."""
    b, want = MK.forest_batch(), MK.forest_expected(40, 3)
    need = len(want["u"])
    cap = need - short
    got = device_map(b, MM.make_params(), chain_cap=cap)
    assert got["intact"] and got["counts"][0] == need and np.array_equal(got["chain_off"], want["chain_off"])
    assert np.array_equal(got["u"], want["u"][:cap]) and np.array_equal(got["n_chained"], want["n_chained"])
    if short == 0:
        same(got, want, b)
    else:
        assert got["counts"][1] == -1 and not got["reg_off"].any() and len(got["regs"]) == 0
        with pytest.raises(N.GbxError) as e:
            host_map(b, MM.make_params(), chain_cap=cap)
        assert e.value.code == N.GBX_ERR_ARG and str(need) in str(e.value)


@pytest.mark.parametrize("short", [0, 1, 100])
def test_region_capacity(short):
    b, want = MK.forest_batch(), MK.forest_expected(40, 3)
    need = len(want["regs"]["id"])
    cap = need - short
    got = device_map(b, MM.make_params(), reg_cap=cap)
    assert got["intact"] and got["counts"] == (len(want["u"]), need)
    assert np.array_equal(got["reg_off"], want["reg_off"]) and np.array_equal(got["u"], want["u"]) and len(got["regs"]) == cap
    for k in MR.REG_FIELDS:
        assert np.array_equal(got["regs"][k].astype(np.int64), want["regs"][k][:cap]), k
    if short:
        with pytest.raises(N.GbxError) as e:
            host_map(b, MM.make_params(), reg_cap=cap)
        assert e.value.code == N.GBX_ERR_ARG and str(need) in str(e.value)


def _tseq_off(refs):
    return np.concatenate([[0], np.cumsum([len(r) for r in refs])]).astype(np.int64)


def test_paf_host_and_text_capacity():
    """The text of the restatement's regions, byte for byte; text_cap in the middle of a line: the need, the head, nothing behind it,
    line_off true (the device entry, on the regions a device call left)"""
    import torch
    c = MK.map_case()
    b, e = c["batch"], c["exp"]
    regs = np.zeros(len(e["regs"]["id"]), MM.REG_DTYPE)
    for k in MR.REG_FIELDS:
        regs[k] = e["regs"][k]
    text, line_off = MM.paf_host(regs, e["reg_off"], c["qnames"], b["seq_off"], b["rep_len"], c["tnames"], _tseq_off(c["refs"]))
    assert text.decode() == c["paf"] and line_off[-1] == len(text) and line_off[0] == 0
    lines = c["paf"].split("\n")
    assert all(c["paf"][int(line_off[r]):].startswith(c["qnames"][r] + "\t") for r in range(len(c["reads"])) if e["reg_off"][r] < e["reg_off"][r + 1])
    with pytest.raises(N.GbxError) as err:
        MM.paf_host(regs, e["reg_off"], c["qnames"], b["seq_off"], b["rep_len"], c["tnames"], _tseq_off(c["refs"]), text_cap=len(text) - 1)
    assert err.value.code == N.GBX_ERR_ARG and str(len(text)) in str(err.value) and len(lines) == len(regs) + 1
    got = device_map(b, MM.make_params())
    d_regs, d_reg_off, d_cnt, d_so, d_rep = got["keep"]
    d = dev()
    t = lambda a: torch.from_numpy(a).to(d)
    qn, qo = MM.pack_names(c["qnames"])
    tn, to = MM.pack_names(c["tnames"])
    qn, qo, tn, to, tso = t(qn), t(qo), t(tn), t(to), t(_tseq_off(c["refs"]))
    cap = len(text) - 150
    out = torch.from_numpy(np.full(cap + 64, 0x5a, np.uint8)).to(d)
    lo, nt = torch.full((len(c["reads"]) + 1,), -7, dtype=torch.int64, device=d), torch.full((1,), -7, dtype=torch.int64, device=d)
    L = MM.lib()
    wb = L.gbx_mm_paf_workspace_bytes(len(c["reads"]), len(regs))
    work = torch.empty(wb, dtype=torch.uint8, device=d)
    N.check(L.gbx_mm_paf_device(len(c["reads"]), d_regs.data_ptr(), d_reg_off.data_ptr(), d_cnt.data_ptr() + 8, len(regs), qn.data_ptr(), qo.data_ptr(),
                                d_so.data_ptr(), d_rep.data_ptr(), len(c["refs"]), tn.data_ptr(), to.data_ptr(), tso.data_ptr(), out.data_ptr(), cap,
                                lo.data_ptr(), nt.data_ptr(), work.data_ptr(), wb, stream()))
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert int(nt.item()) == len(text) and np.array_equal(lo.cpu().numpy(), line_off)
    assert o[:cap].tobytes() == text[:cap] and (o[cap:] == 0x5a).all()


@pytest.fixture(scope="module")
def mapper():
    c = MK.map_case()
    ix = MS.DeviceMmIndex(MS.make_params(**MK.MAP_PARAMS), c["refs"], dev(), stream())
    m = MM.DeviceMmMapper(MS.DeviceMmSeeder(ix, c["reads"]), read_names=c["qnames"], ref_names=c["tnames"])
    m.run(stream())
    return m


def test_mapper_end_to_end(mapper):
    """reads -> seeds -> chain scores -> chains -> regions -> PAF on one stream, equal to the restatement of everything (mm_ref's
    seeding, the chain oracle, mm_map_ref), the text byte for byte"""
    c = MK.map_case()
    e = c["exp"]
    assert mapper.fits() and mapper.counts() == (len(e["u"]), len(e["regs"]["id"]), len(c["paf"]))
    got = mapper.results()
    same(got, e, c["batch"])
    assert mapper.paf() == c["paf"]
    lo = got["line_off"]
    assert lo[0] == 0 and lo[-1] == len(c["paf"]) and (np.diff(lo) >= 0).all()


def test_two_runs_are_identical(mapper):
    first, text = mapper.results(), mapper.paf()
    mapper.run(stream())
    again = mapper.results()
    for k in ("chain_off", "u", "n_chained", "reg_off", "line_off"):
        assert np.array_equal(first[k], again[k]), k
    assert first["regs"].tobytes() == again["regs"].tobytes() and mapper.paf() == text
    c = MK.map_case()
    for r in range(len(c["reads"])):
        lo, hi = int(c["batch"]["off"][r]), int(c["batch"]["off"][r]) + int(first["n_chained"][r])
        assert np.array_equal(first["cax"][lo:hi], again["cax"][lo:hi]) and np.array_equal(first["cay"][lo:hi], again["cay"][lo:hi])


def test_mapper_reports_a_capacity(mapper):
    c = MK.map_case()
    m = MM.DeviceMmMapper(mapper.seeder, read_names=c["qnames"], ref_names=c["tnames"], reg_cap=len(c["exp"]["regs"]["id"]) - 1)
    m.run(stream())
    assert not m.fits() and m.counts()[1] == len(c["exp"]["regs"]["id"])
    with pytest.raises(N.GbxError):
        m.paf()


def test_mmpaf_driver(tmp_path):
    """mmpaf on the mapped reads written to files gives the text of the restatement (names cut at the first blank)"""
    c = MK.map_case()
    fa, fq, out = tmp_path / "ref.fa", tmp_path / "reads.fq", tmp_path / "out.paf"
    with open(fa, "w") as f:
        for nm, r in zip(c["tnames"], c["refs"]):
            f.write(">%s some text\n" % nm)
            f.write("\n".join(r[o:o + 70].decode() for o in range(0, len(r), 70)) + "\n")
    with open(fq, "w") as f:
        for nm, r in zip(c["qnames"], c["reads"]):
            f.write("@%s\tmore\n%s\n+\n%s\n" % (nm, r.decode(), "I" * len(r)))
    r = subprocess.run([os.path.join(BIN, "mmpaf"), "--mid-occ", str(MK.MAP_PARAMS["mid_occ"]), "-o", str(out), str(fa), str(fq)], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "Mapping: %d reads" % len(c["reads"]) in r.stderr and "%d mappings" % len(c["exp"]["regs"]["id"]) in r.stderr
    assert open(out).read() == c["paf"]
    r = subprocess.run([os.path.join(BIN, "mmpaf"), "--mid-occ", "20", "-N", "0", str(fa), str(fq)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "tp:A:S" not in r.stdout and r.stdout.count("\n") == int((c["exp"]["regs"]["parent"] == c["exp"]["regs"]["id"]).sum())


# ------------------------------------------------------------------------------------------------ the scans' block edges
SCAN_BLOCK = 1024                                            # the entries a block of the scan takes (the threads of the one-block scan)


@functools.lru_cache(maxsize=None)
def padded_forests(n_reads):
    """The forest batch among empty reads (no anchors), n_reads in all: four real reads in front, eight up to the last but one - across
    entry 1024 of the offsets where n_reads reaches it - and one last.  -> (batch, the restatement's answer on it)"""
    b = MK.forest_batch()
    k = len(b["off"]) - 1
    pos = np.array(list(range(4)) + list(range(n_reads - 1 - (k - 5), n_reads - 1)) + [n_reads - 1])
    assert len(pos) == k and (np.diff(pos) > 0).all() and pos[-1] == n_reads - 1

    def spread(per_read, fill, dt):
        out = np.full(n_reads, fill, dt)
        out[pos] = per_read
        return out
    offs = lambda per_read: np.concatenate([[0], np.cumsum(per_read)]).astype(np.int64)
    pb = dict(b, off=offs(spread(np.diff(b["off"]), 0, np.int64)), qlen=spread(b["qlen"], 100, np.int64), rep_len=spread(b["rep_len"], 0, np.int32),
              hash=spread(b["hash"], 0, np.uint32))
    pb["seq_off"] = offs(pb["qlen"])
    want = MK.expected(pb, min_chain_score=40, min_cnt=3)
    flat = MK.forest_expected(40, 3)                              # the padding shifts the offsets and the regions' reads, nothing else
    assert np.array_equal(want["u"], flat["u"]) and np.array_equal(want["regs"]["read"], pos[flat["regs"]["read"]])
    assert np.array_equal(np.diff(want["reg_off"])[pos], np.diff(flat["reg_off"])) and want["reg_off"][-1] == flat["reg_off"][-1]
    return pb, want


@pytest.mark.parametrize("n_reads", [SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1])
def test_map_scans_at_the_block_edge(n_reads):
    """chain_off and reg_off of n_reads + 1 entries fill a scan block exactly, pass it by one and by two: both scans, u, the regions and
    both counts equal the restatement's shifted by the padding; at 1 025 reads a chain_cap one short still means no regions"""
    b, want = padded_forests(n_reads)
    got = device_map(b, MM.make_params())
    assert got["intact"] and got["counts"] == (len(want["u"]), len(want["regs"]["id"]))
    same(got, want, b)
    if n_reads == SCAN_BLOCK + 1:
        short = device_map(b, MM.make_params(), chain_cap=len(want["u"]) - 1)
        assert short["intact"] and short["counts"] == (len(want["u"]), -1) and np.array_equal(short["chain_off"], want["chain_off"])
        assert not short["reg_off"].any() and short["reg_off"].shape == (n_reads + 1,)


@pytest.mark.parametrize("reg_cap", [None, SCAN_BLOCK, SCAN_BLOCK + 1], ids=["need", "1024", "1025"])
def test_paf_device_scan_at_the_block_edge(reg_cap):
    """gbx_mm_paf_device with room for more regions than there are, up to and past a scan block: the recorded text byte for byte,
    n_text and line_off true, nothing behind text_cap"""
    c = MK.map_case()
    e = c["exp"]
    regs = np.zeros(len(e["regs"]["id"]), MM.REG_DTYPE)
    for k in MR.REG_FIELDS:
        regs[k] = e["regs"][k]
    assert 0 < len(regs) < SCAN_BLOCK
    text = c["paf"].encode()
    ends = np.concatenate([[0], np.cumsum([len(ln) + 1 for ln in c["paf"].split("\n")[:-1]])])
    got = MK.device_paf(regs, e["reg_off"], c["qnames"], c["batch"]["seq_off"], c["batch"]["rep_len"], c["tnames"], _tseq_off(c["refs"]),
                        len(regs) if reg_cap is None else reg_cap, len(text))
    assert got["n_text"] == len(text) and got["text"] == text and got["intact"]
    assert np.array_equal(got["line_off"], ends[e["reg_off"]])
