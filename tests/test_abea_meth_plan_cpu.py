"""CPU-side checks for the call-methylation site planner and job order on the device: the new symbols, the argument errors that come
before any device work, the tables half of the plan, the hand-made cases of tests/abea_meth_plan_cases.py against the host planner
(each is what it claims), the call-methylation TSV writer, and the planner's rules (csrc/abea_meth_rules.h) compiled for the host in
a stand-alone program under ASan + UBSan (tests/sanitize_abea_meth) against the host planner."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abea_meth_plan_cases as K  # noqa: E402
import abea_meth_ref as R  # noqa: E402
from genomicsbench_amd import _native as N  # noqa: E402
from genomicsbench_amd import abea_meth as AM  # noqa: E402
from genomicsbench_amd.abea import PAIR_DTYPE  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "abea_meth.npz")
SAN = os.path.join(ROOT, "tests", "sanitize_abea_meth")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_symbols_exported():
    L = AM._lib()
    for name in ("gbx_abea_meth_sites_work", "gbx_abea_meth_sites_device", "gbx_abea_meth_tables_host", "gbx_abea_meth_order_work",
                 "gbx_abea_meth_order_device", "gbx_abea_meth_tsv_host"):
        assert hasattr(L, name), name
    for name in ("tables_host", "tsv_host", "DeviceAbeaMethSites"):
        assert hasattr(AM, name), name
    assert hasattr(AM.DeviceAbeaMethJobSet, "from_device")
    assert L.gbx_abea_meth_sites_work(1025, 100) >= 2 * 2 * 8 and L.gbx_abea_meth_sites_work(-1, 0) == 0 and L.gbx_abea_meth_sites_work(1, -1) == 0
    assert L.gbx_abea_meth_order_work(1000) >= 1000 * 24 and L.gbx_abea_meth_order_work(-1) == 0 and L.gbx_abea_meth_order_work(0) > 0


def test_argument_errors_come_first():
    """refused on the arguments alone: these pass without a device"""
    L = AM._lib()
    one = 1                                                # stands for a device pointer that is never followed
    A = N.GBX_ERR_ARG
    sites = lambda pass_, n, site_cap=0, seq_cap=0, work=one, sites_=None: L.gbx_abea_meth_sites_device(
        pass_, n, one, one, one, one, one, one, one, work, one, one, one, site_cap, sites_, sites_, seq_cap, None, None)
    assert sites(0, 1) == A and sites(4, 1) == A and sites(1, -1) == A and sites(1, 1, -1) == A and sites(1, 1, 0, -1) == A
    assert sites(1, 1, work=None) == A and "null" in N.lib().gbx_last_error().decode()
    assert sites(2, 1, site_cap=1) == A                    # a fill with room for a site and nowhere to put it
    assert sites(1, 0, work=None) == 0 and sites(3, 0) == 0
    order = lambda nj, flank=2, bits=1, work=one, tail=one, seq_bytes=0, n_reads=1: L.gbx_abea_meth_order_device(
        nj, one, seq_bytes, n_reads, one, flank, bits, work, one, tail, tail, None)
    assert order(-1) == A and order(1, flank=1) == A and order(1, bits=0) == A and order(1, bits=31) == A and order(1, flank=3, bits=1) == A
    assert order(1, seq_bytes=-1) == A and order(1, n_reads=-1) == A
    assert order(1, work=None) == A and order(0, tail=None) == A
    z = np.zeros(4, np.float32)
    assert L.gbx_abea_meth_tables_host(1, None, N.ptr(z), N.ptr(z), 2, N.ptr(z), N.ptr(z)) == A
    assert L.gbx_abea_meth_tables_host(0, None, N.ptr(np.zeros(AM.FLOGSUM_TBL, np.float32)), None, 1, N.ptr(z), N.ptr(z)) == A       # flank_len < 2
    nb = np.zeros(1, np.int64)
    assert L.gbx_abea_meth_tsv_host(0, None, None, 0, None, None, None, None, None, None, 3, -1, -1, 0, 0, None, N.ptr(nb)) == A      # version
    assert L.gbx_abea_meth_tsv_host(0, None, None, 0, None, None, None, None, None, None, 1, -1, -1, 0, 0, None, None) == A
    assert L.gbx_abea_meth_tsv_host(1, None, None, 0, None, None, None, None, None, None, 1, -1, -1, 0, 0, None, N.ptr(nb)) == A
    assert L.gbx_abea_meth_tsv_host(0, None, None, 0, None, None, None, None, None, None, 1, -1, -1, 0, 0, None, N.ptr(nb)) == 0 and nb[0] == 0


def test_tables_host_equals_plan_host():
    js = R.edge_job_set()
    p = js.plan()
    flank_len = len(p["pre_flank"])
    t = AM.tables_host(js.events_per_base, flank_len)
    for k in ("flogsum", "trans", "pre_flank", "post_flank"):
        assert t[k].shape == p[k].shape and np.array_equal(_bits(t[k]), _bits(p[k])), k
    longer = AM.tables_host(js.events_per_base, flank_len + 1000)                          # a longer table starts with the shorter one
    assert np.array_equal(_bits(longer["pre_flank"][:flank_len]), _bits(p["pre_flank"]))
    assert np.array_equal(_bits(longer["post_flank"][:flank_len]), _bits(p["post_flank"]))
    assert len(AM.tables_host(np.zeros(0), 2)["pre_flank"]) == 2


def test_cases_are_what_they_claim():
    cs = K.cases()
    assert len({c.name for c in cs}) == len(cs)
    sites, jobs, arena = AM.sites_host(*K.planner_args(K.edge_batch()))
    for r, c in enumerate(cs):
        mine = sites[sites["read"] == r]
        got = [(int(s["start_position"]) - c.pos, int(s["end_position"]) - c.pos, int(s["n_cpg"])) for s in mine]
        if isinstance(c.sites, int):
            assert len(got) == c.sites, c.name
        elif c.sites is None:
            assert len(got) > 10 and max(g[2] for g in got) >= 2, c.name
        else:
            assert got == list(c.sites), c.name
        if c.seq_len is not None:
            assert jobs["seq_len"][0::2][sites["read"] == r].tolist() == c.seq_len, c.name
        # alone, the read gives what it gives in the batch: no case leans on its neighbours
        alone = AM.sites_host(*K.planner_args(K.batch([c])))[0]
        assert np.array_equal(alone[["start_position", "end_position", "n_cpg", "ctx_off", "ctx_len"]],
                              mine[["start_position", "end_position", "n_cpg", "ctx_off", "ctx_len"]]), c.name
    by = {c.name: r for r, c in enumerate(cs)}
    j = jobs[0::2][sites["read"] == by["reverse"]]
    assert j["rc"].tolist() == [1] and j["event_start"][0] > j["event_stop"][0]
    j = jobs[0::2][sites["read"] == by["diff11"]]
    assert abs(int(j["event_stop"][0]) - int(j["event_start"][0])) == 11
    assert max(np.bincount(sites["read"])) > 64
    # the restatement agrees on the whole batch
    want = R.sites(*K.planner_args(K.edge_batch()))
    assert np.array_equal(sites, want[0]) and np.array_equal(jobs, want[1]) and np.array_equal(arena, want[2])
    for n in (1023, 1024, 1025):
        s = AM.sites_host(*K.planner_args(K.tiny_batch(n)))[0]
        assert len(s) == n - n // 3 - (1 if n % 3 == 2 else 0) and set(np.flatnonzero(np.bincount(s["read"], minlength=n) == 0) % 3) == {1}


# ------------------------------------------------------------------------------------------------ TSV
def _golden_tsv_inputs():
    g = np.load(GOLDEN)
    ref_off = np.concatenate([[0], np.cumsum(g["ref_len"])[:-1]]).astype(np.int64)
    sites = AM.sites_host(ref_off, g["ref_len"], g["ref_arena"], g["ref_start_pos"], g["rc"], g["rec_off"], g["rec"].copy().view(PAIR_DTYPE).reshape(-1))[0]
    scores = np.stack([g["site_unmeth"].view(np.float32), g["site_meth"].view(np.float32)], axis=1).copy()
    scores[3] = (-101.25, -101.25)                         # equal scores: 0.00
    scores[4] = (-87.5, -87.50390625)                      # methylated - unmethylated = -0.0039: rounds to -0.00
    names = ["read_%d" % r for r in range(5)]
    contigs = ["chr20", "chr20", "chrX", "chr20", "chrM"]
    return g, ref_off, sites, scores, names, contigs


def _tsv_lines(g, ref_off, sites, scores, names, contigs, version, clip_start, clip_end):
    out = []
    for s, (u, m) in zip(sites, scores):
        r = int(s["read"])
        if (clip_start != -1 and s["start_position"] < clip_start) or (clip_end != -1 and s["end_position"] >= clip_end):
            continue
        ref = R.disambiguate(bytes(g["ref_arena"][ref_off[r]:ref_off[r] + g["ref_len"][r]]))
        ctx = ref[s["ctx_off"]:s["ctx_off"] + s["ctx_len"]].decode()
        strand = "%s\t" % ("-" if g["rc"][r] else "+") if version == 2 else ""
        out.append("%s\t%s%d\t%d\t%s\t%.2f\t%.2f\t%.2f\t1\t%d\t%s\n" % (contigs[r], strand, s["start_position"], s["end_position"], names[r],
                                                                     float(m) - float(u), float(m), float(u), s["n_cpg"], ctx))
    return out


HEADERS = {1: "chromosome\tstart\tend\tread_name\tlog_lik_ratio\tlog_lik_methylated\tlog_lik_unmethylated\tnum_calling_strands\tnum_cpgs\tsequence\n",
           2: "chromosome\tstrand\tstart\tend\tread_name\tlog_lik_ratio\tlog_lik_methylated\tlog_lik_unmethylated\tnum_calling_strands\tnum_motifs\tsequence\n"}


@pytest.mark.parametrize("version", [1, 2])
@pytest.mark.parametrize("header", [False, True])
def test_tsv_on_the_golden_sites(version, header):
    g, ref_off, sites, scores, names, contigs = _golden_tsv_inputs()
    assert len(sites) == 398
    args = (sites, scores, names, contigs, g["rc"], ref_off, g["ref_len"], g["ref_arena"])
    want = "".join(_tsv_lines(g, ref_off, sites, scores, names, contigs, version, -1, -1))
    got = AM.tsv_host(*args, version=version, with_header=header).decode()          # the sizing call, then a buffer of exactly that size
    assert got == (HEADERS[version] if header else "") + want
    assert "\t0.00\t-101.25\t-101.25\t" in got and "\t-0.00\t-87.50\t-87.50\t" in got
    # a window that cuts sites at both ends, per read (positions are per contig; the rule is applied to every site as written)
    lo, hi = int(np.sort(sites["start_position"])[40]), int(np.sort(sites["end_position"])[-40])
    cut = _tsv_lines(g, ref_off, sites, scores, names, contigs, version, lo, hi)
    assert 0 < len(cut) < len(sites) - 60
    assert AM.tsv_host(*args, version=version, clip_start=lo, clip_end=hi, with_header=header).decode() == (HEADERS[version] if header else "") + "".join(cut)
    only_start = _tsv_lines(g, ref_off, sites, scores, names, contigs, version, lo, -1)
    assert AM.tsv_host(*args, version=version, clip_start=lo).decode() == "".join(only_start) and len(only_start) > len(cut)
    # one byte short: GBX_ERR_ARG with the need
    with pytest.raises(N.GbxError) as e:
        AM.tsv_host(*args, version=version, with_header=header, cap=len(got) - 1)
    assert e.value.code == N.GBX_ERR_ARG and str(len(got)) in str(e.value)
    assert AM.tsv_host(*args, version=version, with_header=header, cap=len(got)).decode() == got
    assert AM.tsv_host(sites[:0], scores[:0], names, contigs, g["rc"], ref_off, g["ref_len"], g["ref_arena"], version=version, with_header=True).decode() == HEADERS[version]


def test_tsv_refuses_sites_outside_their_reads():
    g, ref_off, sites, scores, names, contigs = _golden_tsv_inputs()
    for field, value in (("read", 5), ("read", -1), ("ctx_off", -1), ("ctx_len", 1 << 20)):
        bad = sites[:3].copy()
        bad[field][1] = value
        with pytest.raises(N.GbxError) as e:
            AM.tsv_host(bad, scores[:3], names, contigs, g["rc"], ref_off, g["ref_len"], g["ref_arena"])
        assert e.value.code == N.GBX_ERR_ARG and "site 1" in str(e.value)


# ------------------------------------------------------------------------------------------------ sanitizers
def test_rules_under_asan_ubsan(tmp_path):
    """The rules the kernels compile, built for the host in a stand-alone program under ASan + UBSan, on the edge batch and a batch at
    the scan's block edge, every buffer exactly as large as needed: clean, and the host planner's bytes."""
    r = subprocess.run(["make", "-C", SAN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for name, b in (("edge", K.edge_batch()), ("tiny", K.tiny_batch(1025))):
        src, out = tmp_path / (name + ".bin"), tmp_path / (name + ".out")
        with open(src, "wb") as f:
            f.write(np.array([len(b["ref_len"]), b["ref_arena"].size, len(b["rec"])], np.int64).tobytes())
            for k in ("ref_off", "ref_len", "ref_start_pos", "rc", "rec_off", "ref_arena", "rec"):
                f.write(np.ascontiguousarray(b[k]).tobytes())
        r = subprocess.run([os.path.join(SAN, "_build", "meth_main"), str(src), str(out)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
        raw = open(out, "rb").read()
        ns, nb = (int(v) for v in np.frombuffer(raw[:16], np.int64))
        sites, jobs, arena = AM.sites_host(*K.planner_args(b))
        assert (ns, nb) == (len(sites), len(arena)) and ns > 0
        at = 16
        assert raw[at:at + 32 * ns] == sites.tobytes()
        at += 32 * ns
        assert raw[at:at + 80 * ns] == jobs.tobytes()
        at += 80 * ns
        assert raw[at:] == arena.tobytes()
