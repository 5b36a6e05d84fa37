"""pileup on the GPU: the layout and counts of the host and device entries against the CPU restatement (pileup_ref.py),
slicing, several devices, gaps and empty regions, a missing DT, and bin/pileup --print against a table built from the
restatement."""
import os
import subprocess

import numpy as np
import pytest

import pileup_ref as PR
from genomicsbench_amd import _native as N
from genomicsbench_amd import pileup as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "genomicsbench_amd", "bin", "pileup")
DT = ["r941", "r10"]


@pytest.fixture(scope="module")
def bams(tmp_path_factory):
    from genomicsbench_amd.datagen import gen_pileup_preset, gen_pileup_reads
    d = tmp_path_factory.mktemp("pileup")
    out = {}
    c, r = gen_pileup_reads(40000, 15, 11, mean_len=2500, adversarial=True)
    out["adv"] = str(d / "adv.bam")
    P.write_bam(out["adv"], c, r)
    c, r = gen_pileup_preset("small", workers=8)
    out["small"] = str(d / "small.bam")
    P.write_bam(out["small"], c, r)
    c, r = gen_pileup_reads(300000, 1.5, 12, mean_len=3000)           # coverage gaps
    out["gaps"] = str(d / "gaps.bam")
    P.write_bam(out["gaps"], c, r)
    c, r = gen_pileup_reads(230000, 8, 13, mean_len=3000, adversarial=True)
    out["print"] = str(d / "print.bam")
    P.write_bam(out["print"], c, r)
    c, r = gen_pileup_reads(30000, 6, 14, mean_len=2000, missing_dt=3)
    out["nodt"] = str(d / "nodt.bam")
    P.write_bam(out["nodt"], c, r)
    return out


def _check_against_ref(bam, region, nd, nh):
    rs, (_, beg, end) = P.read_bam(bam, region, DT[:nd] if nd > 1 else None)
    want_pc, want_st = PR.layout(rs, beg, end, nd)
    pc, st = P.layout_host(rs, beg, end, nd, nh)
    assert np.array_equal(pc, want_pc)
    assert st == want_st
    want = PR.counts(rs, beg, end, pc, nd, nh)
    got = P.count_host(rs, beg, end, pc, num_dtypes=nd, num_homop=nh)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    return rs, beg, end, pc, got


@pytest.mark.parametrize("nd,nh", [(1, 1), (1, 5), (2, 1), (2, 5)])
def test_adversarial_matches_restatement(bams, nd, nh):
    _check_against_ref(bams["adv"], "ctg1", nd, nh)


@pytest.mark.parametrize("nd,nh", [(1, 1), (1, 5), (2, 1), (2, 5)])
def test_small_matches_restatement(bams, nd, nh):
    # a 60 kb stretch of 'small' (the restatement walks reads in Python) ...
    _check_against_ref(bams["small"], "ctg1:700,001-760,000", nd, nh)


def test_small_whole_contig_layout(bams):
    # ... and the layout of the whole contig (cheap to restate)
    rs, (_, beg, end) = P.read_bam(bams["small"], "ctg1", DT)
    pc, st = P.layout_host(rs, beg, end, 2, 5)
    want_pc, want_st = PR.layout(rs, beg, end, 2)
    assert np.array_equal(pc, want_pc) and st == want_st


def test_device_entries_equal_host(bams):
    import torch
    rs, (_, beg, end) = P.read_bam(bams["small"], "ctg1", DT)
    pc, st = P.layout_host(rs, beg, end, 2, 5)
    host = P.count_host(rs, beg, end, pc, num_dtypes=2, num_homop=5)
    d = P.DevicePileup(rs, "cuda:0", beg, end, 2, 5)
    s = torch.cuda.current_stream().cuda_stream
    d.layout(s)
    torch.cuda.synchronize()
    dpc, dst = d.layout_results()
    assert np.array_equal(dpc, pc) and dst == st
    d.alloc_counts(st["n_cols"])
    d.count(stream=s)
    torch.cuda.synchronize()
    for g, w in zip(d.count_results(st["n_cols"]), host):
        assert np.array_equal(g, w)
    # a sub-range of positions: the matching slice of the whole
    p0, p1 = beg + 400000, beg + 650000
    d.count(p0, p1, stream=s)
    torch.cuda.synchronize()
    c0, c1 = int(pc[p0 - beg]), int(pc[p1 - beg])
    got = d.count_results(c1 - c0)
    for g, w in zip(got, host):
        assert np.array_equal(g, w[c0:c1])


def test_slices_and_devices_equal_default(bams):
    rs, (_, beg, end) = P.read_bam(bams["small"], "ctg1")
    base = P.pileup_host(rs, beg, end, 1, 5)
    sliced = P.pileup_host(rs, beg, end, 1, 5, slice_positions=1000)
    for g, w in zip(sliced, base):
        assert (g == w) if isinstance(w, dict) else np.array_equal(g, w)
    saved = os.environ.get("GBX_DEVICE_MAP")
    os.environ["GBX_DEVICE_MAP"] = "0,0,0"
    try:
        N.check(N.lib().gbx_host_set_devices(3))
        multi = P.pileup_host(rs, beg, end, 1, 5, slice_positions=100000)
    finally:
        N.check(N.lib().gbx_host_set_devices(0))
        if saved is None:
            os.environ.pop("GBX_DEVICE_MAP", None)
        else:
            os.environ["GBX_DEVICE_MAP"] = saved
    for g, w in zip(multi, base):
        assert (g == w) if isinstance(w, dict) else np.array_equal(g, w)
    # a count sub-range through the host entry equals the slice of the whole
    pc = base[0]
    p0, p1 = beg + 123457, beg + 987654
    c0, c1 = int(pc[p0 - beg]), int(pc[p1 - beg])
    part = P.count_host(rs, beg, end, pc, p0, p1, 1, 5, slice_positions=77777)
    for g, w in zip(part, base[2:]):
        assert np.array_equal(g, w[c0:c1])


def test_gaps_and_empty_regions(bams):
    rs, beg, end, pc, _ = _check_against_ref(bams["gaps"], "ctg1", 1, 5)
    assert (np.diff(pc) == 0).any()                                    # positions without columns exist
    rs, _ = P.read_bam(bams["gaps"], "ctg1")
    for a, b in ((5000, 5000), (0, 0), (299999, 300000)):
        pc, st = P.layout_host(rs, a, b, 1, 5)
        want_pc, want_st = PR.layout(rs, a, b, 1)
        assert np.array_equal(pc, want_pc) and st == want_st
        got = P.count_host(rs, a, b, pc, num_dtypes=1, num_homop=5)
        for g, w in zip(got, PR.counts(rs, a, b, pc, 1, 5)):
            assert np.array_equal(g, w)
    empty = P.PileupReads.from_records([])
    pc, st = P.layout_host(empty, 100, 200, 1, 5)
    assert not pc.any() and st["n_cols"] == 0


def test_missing_dtype_is_an_error(bams):
    rs, (_, beg, end) = P.read_bam(bams["nodt"], "ctg1", DT)
    assert (rs.dtype < 0).sum() == 3
    with pytest.raises(N.GbxError) as e:
        P.layout_host(rs, beg, end, 2, 5)
    assert e.value.code == N.GBX_ERR_ARG
    pc, _ = P.layout_host(rs, beg, end, 1, 5)                     # one dtype: DT is not looked at
    with pytest.raises(N.GbxError):
        P.count_host(rs, beg, end, pc, num_dtypes=2, num_homop=5)
    import ctypes as C
    cr = rs.c_struct()
    with pytest.raises(N.GbxError) as e:                           # Weibull summation is not built
        N.check(N.lib().gbx_pileup_layout_host(C.byref(P.make_params(beg, end, 1, 5, weibull=1)), C.byref(cr),
                                               N.ptr(np.zeros(end - beg + 1, dtype=np.int64)), C.byref(P.LayoutStats())))
    assert e.value.code == N.GBX_ERR_UNSUPPORTED
    r = subprocess.run([BIN, bams["nodt"], "ctg1", "2"] + DT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "Datatype not found for read_" in r.stderr, r.stderr


def _expected_print(bam, region, dtypes):
    nd = max(1, len(dtypes))
    rs, (name, beg, end) = P.read_bam(bam, region, dtypes if nd > 1 else None)
    batches = P.driver_batches(name, beg, end)
    lo, hi = batches[0][1], end
    rs, _ = P.read_bam(bam, "%s:%d-%d" % (name, lo + 1, hi), dtypes if nd > 1 else None)
    pc, _ = PR.layout(rs, lo, hi, nd)
    out = []
    for _, a, b in batches:
        major, minor, cnt = PR.counts(rs, lo, hi, pc, nd, 5, a, b)
        buf = P.buffer_cols(np.diff(pc[a - lo:b - lo + 1]), a, b)
        out.append(P.format_batch(major, minor, cnt, nd, 5, dtypes, buf))
    return "".join(out), len(batches)


@pytest.mark.parametrize("group", [None, "1"])
@pytest.mark.parametrize("dtypes", [[], DT])
def test_driver_print_equals_restatement(bams, dtypes, group):
    """group "1": every batch a group of its own (GBX_PILEUP_GROUP_POSITIONS), so the columns of the position two batches
    share are carried from one count call to the next"""
    want, n_batches = _expected_print(bams["print"], "ctg1:1-230000", dtypes)
    env = dict(os.environ)
    if group:
        env["GBX_PILEUP_GROUP_POSITIONS"] = group
    for t in ("1", "4"):
        r = subprocess.run([BIN, bams["print"], "ctg1:1-230000", t] + dtypes + ["--print"], capture_output=True, text=True, timeout=600,
                           env=env)
        assert r.returncode == 0, r.stderr
        assert "Running %d batches with threads: %s" % (n_batches, t) in r.stderr
        assert "Kernel runtime: " in r.stderr
        assert r.stdout == want


def test_driver_print_across_groups_with_gaps(bams):
    """a sparse contig, one batch per group, the region placed so that the position the first two batches share has no
    column: the carried range is empty there, and is not elsewhere"""
    rs, _ = P.read_bam(bams["gaps"], "ctg1")
    pc, _ = PR.layout(rs, 0, 300000, 1)
    gap = next(q for q in range(100000, 150000) if pc[q + 1] == pc[q])
    beg0 = gap - 99999                                   # batch 1 covers [beg0 + 99999, ...): it starts at the gap
    region = "ctg1:%d-%d" % (beg0 + 1, beg0 + 250000)
    want, n_batches = _expected_print(bams["gaps"], region, [])
    assert n_batches == 3
    r = subprocess.run([BIN, bams["gaps"], region, "2", "--print"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, GBX_PILEUP_GROUP_POSITIONS="1"))
    assert r.returncode == 0, r.stderr
    assert r.stdout == want
