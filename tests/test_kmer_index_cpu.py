"""CPU tests of the kmer-cnt minimizer index (no GPU): the literal restatement (tests/kmer_index_ref.py) against the reference's
printed numbers; the product's rules header (csrc/kmer_index_rules.h, built for the host by tests/hostcheck/kmer_index_check.cpp)
against the restatement on the edge cases of tests/kmer_index_cases.py and on generated reads; the tiling constants, the
global-position formula and the fp32 filter at their edges; the driver's config handling; the exported symbols."""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest

from genomicsbench_amd import kmer as K
import kmer_index_cases as KC
import kmer_index_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BIN = os.path.join(ROOT, "genomicsbench_amd", "bin", "kmer-cnt")
LIB = os.path.join(ROOT, "genomicsbench_amd", "libgbx.so")
RUNS = json.load(open(os.path.join(GOLDEN, "kmer_index_reference.json")))["runs"]
CASES = KC.all_cases()


@functools.lru_cache(maxsize=None)
def golden_reads(names, min_read=5000):
    return K.read_fasta([os.path.join(GOLDEN, n) for n in names], min_read)


@functools.lru_cache(maxsize=None)
def golden_index(names, k, w, rate):
    return R.index_ref(golden_reads(names), k, w, rate)


def hostcheck_lib():
    src = os.path.join(ROOT, "tests", "hostcheck", "kmer_index_check.cpp")
    out = os.path.join(ROOT, "tests", "hostcheck", "libkmer_index_check.so")
    hdr = os.path.join(ROOT, "genomicsbench_amd", "csrc", "kmer_index_rules.h")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-fPIC", "-shared", src, "-o", out], check=True)
    L = C.CDLL(out)
    vp, i64 = C.c_void_p, C.c_int64
    L.hostcheck_ki_constants.argtypes = [vp]
    L.hostcheck_ki_read_tiles.argtypes = [i64, C.c_int]
    L.hostcheck_ki_read_tiles.restype = i64
    L.hostcheck_ki_hash.argtypes = [C.c_uint64]
    L.hostcheck_ki_hash.restype = C.c_uint64
    L.hostcheck_ki_minimizers.argtypes = [vp, i64, C.c_int, C.c_int, C.c_int, vp, vp, vp]
    L.hostcheck_ki_minimizers.restype = i64
    L.hostcheck_ki_global_pos.argtypes = [C.c_uint64, i64, i64, C.c_int, C.c_int]
    L.hostcheck_ki_global_pos.restype = C.c_uint64
    L.hostcheck_ki_filter.argtypes = [C.c_uint64, C.c_uint64, C.c_float, C.POINTER(C.c_float)]
    L.hostcheck_ki_filter.restype = C.c_uint64
    L.hostcheck_ki_index.argtypes = [vp, vp, vp, i64, C.c_int, C.c_int, C.c_float, vp, C.POINTER(C.c_float), vp, vp, vp]
    L.hostcheck_ki_index.restype = None
    return L


@pytest.fixture(scope="module")
def hostcheck():
    return hostcheck_lib()


def header_minimizers(L, codes, k, w, mode):
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    n = max(0, codes.size - k)
    pos, rev, code = np.zeros(n + 1, dtype=np.int32), np.zeros(n + 1, dtype=np.uint8), np.zeros(n + 1, dtype=np.uint64)
    got = L.hostcheck_ki_minimizers(codes.ctypes.data, codes.size, k, w, mode, pos.ctypes.data, rev.ctypes.data, code.ctypes.data)
    assert got >= 0, "a position was marked by two walks"
    return pos[:got].tolist(), rev[:got].astype(bool).tolist(), [int(c) for c in code[:got]]


def header_index(L, reads, k, w, rate):
    n = reads.n_positions(k) + 1
    out, mean = np.zeros(5, dtype=np.int64), C.c_float()
    kmer, off, pos = np.zeros(n, dtype=np.uint64), np.zeros(n + 1, dtype=np.int64), np.zeros(n, dtype=np.uint64)
    L.hostcheck_ki_index(reads.enc.ctypes.data, reads.read_off.ctypes.data, reads.read_len.ctypes.data, reads.n_reads, k, w, rate,
                         out.ctypes.data, C.byref(mean), kmer.ctypes.data, off.ctypes.data, pos.ctypes.data)
    st = dict(n_chosen=int(out[0]), n_distinct=int(out[1]), repetitive_frequency=int(out[2]), n_selected=int(out[3]), n_entries=int(out[4]),
              mean_frequency=np.float32(mean.value))
    return st, kmer[:out[3]], off[:out[3] + 1], pos[:out[4]]


def same_index(got, want):
    st, kmer, off, pos = got
    wst, wkmer, woff, wpos = want
    for f in st:
        if f == "mean_frequency":
            assert np.float32(st[f]).view(np.uint32) == np.float32(wst[f]).view(np.uint32)
        else:
            assert st[f] == wst[f], f
    assert np.array_equal(kmer, wkmer) and np.array_equal(off, woff) and np.array_equal(pos, wpos)


# ---- the restatement is the reference
@pytest.mark.parametrize("run", RUNS, ids=lambda r: "%s-k%d-w%d" % ("+".join(r["reads"]), r["k"], r["window"]))
def test_ref_equals_reference_numbers(run):
    st = golden_index(tuple(run["reads"]), run["k"], run["window"], run["repeat_kmer_rate"])[0]
    assert st["total_len"] == run["total_sequence"]
    assert (st["repetitive_frequency"], st["n_repetitive_entries"], st["n_selected"], st["n_entries"]) == \
        (run["repetitive_frequency"], run["filtered"], run["selected"], run["index_size"])
    want = ["Mean k-mer frequency: " + run["mean_frequency"], "Repetitive k-mer frequency: %d" % run["repetitive_frequency"],
            "Filtered %d repetitive k-mers (%s)" % (run["filtered"], run["filtered_ratio"]), "Selected k-mers: %d" % run["selected"],
            "K-mer index size: %d" % run["index_size"], "Mean k-mer frequency: " + run["index_mean_frequency"],
            "Minimizer rate: " + run["minimizer_rate"]]
    assert R.debug_lines(st) == want


def test_goldens_cover_the_issue_s_table():
    got = {(tuple(r["reads"]), r["window"], r["k"]): (r["filtered"], r["selected"], r["index_size"]) for r in RUNS}
    ab, a = ("kmer_a.fasta.gz", "kmer_b.fastq.gz"), ("kmer_a.fasta.gz",)
    for key, want in (((ab, 5, 15), (503, 64273, 67190)), ((ab, 5, 17), (465, 65259, 67197)), ((ab, 5, 21), (357, 66402, 67343)),
                      ((a, 1, 4), (2848, 135, 151796)), ((a, 1, 31), (1761, 152146, 152343)), ((a, 2, 4), (0, 122, 101202)),
                      ((a, 2, 31), (901, 101462, 101587)), ((a, 16, 4), (12775, 70, 5041)), ((a, 16, 31), (105, 17968, 17983))):
        assert got[key] == want
    for r in RUNS:                                       # the config fixtures say what the runs used
        cfg = dict(l.strip().split("=") for l in open(os.path.join(GOLDEN, "kmer_min_w%d.cfg" % r["window"])) if "=" in l and l[0] != "#")
        assert int(cfg["minimizer_window"]) == r["window"] and float(cfg["repeat_kmer_rate"]) == r["repeat_kmer_rate"] and cfg["use_minimizers"] == "1"


# ---- the rules header is the restatement
def test_tiling_constants(hostcheck):
    out = np.zeros(8, dtype=np.int64)
    hostcheck.hostcheck_ki_constants(out.ctypes.data)
    assert out.tolist() == [KC.KI_MAX_K, KC.KI_MAX_WINDOW, 256, KC.KI_LANE, KC.KI_WAVE, KC.KI_TILE, KC.KI_MAX_WINDOW, 1 << 40]
    assert KC.KI_WAVE == 64 * KC.KI_LANE and KC.KI_TILE == 256 * KC.KI_LANE and KC.KI_MAX_WINDOW >= 64
    for k in (1, 15, 31):
        for n in (0, 1, KC.KI_TILE - 1, KC.KI_TILE, KC.KI_TILE + 1, 5 * KC.KI_TILE):
            assert hostcheck.hostcheck_ki_read_tiles(n + k, k) == -(-n // KC.KI_TILE)
        assert hostcheck.hostcheck_ki_read_tiles(k - 1, k) == 0 and hostcheck.hostcheck_ki_read_tiles(0, k) == 0


def test_hash(hostcheck):
    for x in (0, 1, (1 << 62) - 1, 0x123456789ABCDEF, (1 << 64) - 1):
        assert hostcheck.hostcheck_ki_hash(x) == R.splitmix64(x)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_header_equals_restatement_on_the_edge_cases(hostcheck, case):
    reads = KC.read_set(case)
    for o, n in zip(reads.read_off.tolist(), reads.read_len.tolist()):
        want = R.read_minimizers(reads.enc[o:o + n], case.k, case.w)
        want = (want[0], [bool(v) for v in want[1]], want[2])
        for mode in (0, 1):
            assert header_minimizers(hostcheck, reads.enc[o:o + n], case.k, case.w, mode) == want
    want = R.index_ref(reads, case.k, case.w, case.rate)
    got = header_index(hostcheck, reads, case.k, case.w, case.rate)
    same_index(got, want)


def test_case_names_are_true():
    """what the search-built and the index cases claim, on the restatement alone"""
    by = {c.name: c for c in CASES}
    for name, b in (("lane", KC.KI_LANE), ("wave", KC.KI_WAVE), ("tile", KC.KI_TILE)):
        c = by["tiles-events-at-%s-end" % name]
        for i, x in enumerate((b - 2, b - 1, b)):
            rs, ex, run = c.reads[3 * i:3 * i + 3]
            assert x in KC.resets(KC.hashes(rs, c.k), c.w)
            assert x in KC.deque_events(KC.hashes(ex, c.k), c.w)["expiry"]
            km = R.read_kmers(run, c.k)[0]
            assert km[x] == 0 and km[x + 1] != 0
    c = by["ties-equal-hash-at-expiry"]
    assert all(x in KC.deque_events(KC.hashes(r, c.k), c.w)["tie_expiry"] for r, x in zip(c.reads, (3, 7, 20)))
    c = by["ties-palindromes"]
    assert all(not any(R.read_kmers(r, c.k)[1]) for r in c.reads[:2])
    c = by["index-only-reversed"]
    st, kmer, off, pos = R.index_ref(KC.read_set(c), c.k, c.w, c.rate)
    assert 0 in kmer.tolist() and all(40 <= p < 80 for p in pos[off[0]:off[1]].tolist())      # AAA only in the first read's reverse complement
    c = by["index-capacity-at-and-above-the-repetitive-frequency"]
    cap = KC.capacities(c.reads, c.k, c.w)
    st, kmer, off, pos = R.index_ref(KC.read_set(c), c.k, c.w, c.rate)
    rf = st["repetitive_frequency"]
    at = [k for k, v in cap.items() if v == rf]
    above = [k for k, v in cap.items() if v == rf + 1]
    assert at and above and set(at) <= set(kmer.tolist()) and not set(above) & set(kmer.tolist())
    c = by["index-everything-repetitive"]
    st, kmer, off, pos = R.index_ref(KC.read_set(c), c.k, c.w, c.rate)
    assert st["n_chosen"] > 0 and kmer.size == 0 and off.tolist() == [0] and pos.size == 0
    c = by["index-one-kmer-many-reads-both-strands"]
    st, kmer, off, pos = R.index_ref(KC.read_set(c), c.k, c.w, c.rate)
    assert kmer.tolist() == [0] and pos.size > 40 and np.all(np.diff(pos.astype(np.int64)) > 0)


def test_header_equals_restatement_on_generated_reads(hostcheck):
    """2000 reads: random, tandem repeats of period 1..6, homopolymer runs; k = 1..11, w = 2..16"""
    rng = np.random.default_rng(2024)
    for i in range(2000):
        k, w, n = int(rng.integers(1, 12)), int(rng.integers(2, 17)), int(rng.integers(0, 160))
        kind = i % 3
        if kind == 0:
            s = KC.rand_read(rng, n)
        elif kind == 1:
            s = np.tile(KC.rand_read(rng, int(rng.integers(1, 7))), n // 2 + 1)[:n]
        else:
            s = KC.rand_read(rng, n)
            for _ in range(3):
                a = int(rng.integers(0, n + 1))
                s[a:a + int(rng.integers(1, 40))] = rng.integers(0, 4)
        want = R.read_minimizers(s, k, w)
        want = (want[0], [bool(v) for v in want[1]], want[2])
        for mode in (0, 1):
            assert header_minimizers(hostcheck, s, k, w, mode) == want, (i, k, w, s.tolist())


def test_global_position_around_2_to_the_32(hostcheck):
    for g in ((1 << 32) - 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 6, (1 << 40) - 200):
        for L, p, k in ((100, 0, 15), (100, 84, 15), (90, 3, 31), (2, 0, 1)):
            assert hostcheck.hostcheck_ki_global_pos(g, L, p, k, 0) == g + p
            assert hostcheck.hostcheck_ki_global_pos(g, L, p, k, 1) == g + L + (L - p - k)
    # (reads of 2^31 bases cannot be built here: the formula's own terms are held at those bases, and index_ref holds the
    # formula against the reference's numbers on the goldens)


def filter_triples():
    """(total, unique, rate): rate * mean within one ulp of an integer on either side; unique + 1 or total above 2^24"""
    out = []
    f32 = np.float32
    for total, unique in ((1053, 999), (67190, 64272), (7, 2), (1 << 20, 3), ((1 << 24) + 1, 5), ((1 << 24) + 3, (1 << 24) + 1), ((1 << 30) + 77, (1 << 24) + 2),
                          ((1 << 39) - 1, (1 << 25) + 1), (3, (1 << 24) + 1)):
        mean = f32(total) / f32(unique + 1)
        for target in (1, 2, 10, 517, 2821):
            r0 = f32(target) / mean
            for r in (r0, np.nextafter(r0, f32(0)), np.nextafter(r0, f32(np.inf)), np.nextafter(np.nextafter(r0, f32(0)), f32(0))):
                if 0 <= float(r) <= 1048576.0:
                    out.append((total, unique, float(r), target))
    return out


def test_filter_scalar_at_the_ulp(hostcheck):
    triples = filter_triples()
    below = above = 0
    for total, unique, rate, target in triples:
        mean = C.c_float()
        rf = hostcheck.hostcheck_ki_filter(total, unique, rate, C.byref(mean))
        wmean, wrf = R.filter_scalar(total, unique, rate)
        assert np.float32(mean.value).view(np.uint32) == np.float32(wmean).view(np.uint32) and rf == wrf, (total, unique, rate)
        assert wrf in (target - 1, target)
        below += wrf == target - 1
        above += wrf == target
    assert below > 10 and above > 10                      # both sides of an integer occur


# ---- the driver
@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    import gzip
    d = tmp_path_factory.mktemp("kmer_index_plain")
    path = str(d / "kmer_a.fasta")
    with gzip.open(os.path.join(GOLDEN, "kmer_a.fasta.gz"), "rb") as f, open(path, "wb") as g:
        g.write(f.read())
    return path


def run_driver(args):
    return subprocess.run([BIN] + args, capture_output=True, text=True)


def test_driver_missing_keys_and_k_range(plain, tmp_path):
    base = "kmer_size=15\nuse_minimizers=1\nassemble_kmer_sample=1\n"
    (tmp_path / "now.cfg").write_text(base + "repeat_kmer_rate=10\n")
    r = run_driver(["--reads", plain, "--config", str(tmp_path / "now.cfg"), "--parse-only"])
    assert r.returncode != 0 and "No such parameter: minimizer_window" in r.stderr
    (tmp_path / "nor.cfg").write_text(base + "minimizer_window=5\n")
    r = run_driver(["--reads", plain, "--config", str(tmp_path / "nor.cfg"), "--parse-only"])
    assert r.returncode != 0 and "No such parameter: repeat_kmer_rate" in r.stderr
    cfg = os.path.join(GOLDEN, "kmer_min_w5.cfg")
    r = run_driver(["--reads", plain, "--config", cfg, "--kmer", "31", "--parse-only", "--debug"])
    assert r.returncode == 0 and "Running with k-mer size: 31" in r.stderr
    r = run_driver(["--reads", plain, "--config", cfg, "--kmer", "32", "--parse-only"])
    assert r.returncode != 0 and "32" in r.stderr
    assert run_driver(["--reads", plain, "--config", cfg, "--kmer", "0", "--parse-only"]).returncode != 0
    # the count path keeps its limit
    assert run_driver(["--reads", plain, "--config", os.path.join(GOLDEN, "kmer_k15.cfg"), "--kmer", "18", "--parse-only"]).returncode != 0
    (tmp_path / "wide.cfg").write_text(base + "minimizer_window=65\nrepeat_kmer_rate=10\n")
    r = run_driver(["--reads", plain, "--config", str(tmp_path / "wide.cfg"), "--parse-only"])
    assert r.returncode != 0 and "minimizer_window" in r.stderr
    r = run_driver(["--reads", plain, "--config", os.path.join(GOLDEN, "kmer_k15.cfg"), "--index", str(tmp_path / "x"), "--parse-only"])
    assert r.returncode != 0 and "--index" in r.stderr


def test_driver_parse_only_unchanged(plain):
    outs = []
    for cfg in ("kmer_k15.cfg", "kmer_min_w5.cfg"):
        r = run_driver(["--reads", plain, "--config", os.path.join(GOLDEN, cfg), "--parse-only"])
        assert r.returncode == 0
        outs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    rs = K.read_fasta(plain, 5000)
    assert outs[0] == outs[1] and (outs[0]["reads"], outs[0]["bases"], outs[0]["fnv1a"]) == (rs.n_reads, rs.n_bases, rs.checksum())


def test_symbols_exported_and_limits():
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout.split()
    for s in ("gbx_kmer_minimizers_host", "gbx_kmer_minimizers_device", "gbx_kmer_index_host", "gbx_kmer_index_device", "gbx_kmer_index_workspace_bytes"):
        assert s in syms
    from genomicsbench_amd import kmer_index as KI
    L = KI._lib()
    assert L.gbx_kmer_index_workspace_bytes(15, 10, 1000, 0) > 2000
    assert L.gbx_kmer_index_workspace_bytes(15, 10, 1000, 1) > L.gbx_kmer_index_workspace_bytes(15, 10, 1000, 0) + 32 * 1000
    assert L.gbx_kmer_index_workspace_bytes(31, 0, 0, 1) > 0
    assert L.gbx_kmer_index_workspace_bytes(32, 10, 1000, 1) == 0 and L.gbx_kmer_index_workspace_bytes(0, 10, 1000, 1) == 0
    assert L.gbx_kmer_index_workspace_bytes(15, 10, 1 << 39, 1) == 0 and L.gbx_kmer_index_workspace_bytes(15, 10, (1 << 39) - 1, 0) > 0


def test_host_entries_refuse_before_the_device():
    """bad k, window, rate, a read outside enc: GBX_ERR_ARG; 2 * total_len at 2^40: GBX_ERR_UNSUPPORTED, naming the limit"""
    from genomicsbench_amd import _native as N
    from genomicsbench_amd import kmer_index as KI
    rs = K.KmerReadSet.from_codes([np.zeros(20, dtype=np.uint8)])
    for kw in (dict(k=0, window=5), dict(k=32, window=5), dict(k=5, window=0), dict(k=5, window=65), dict(k=5, window=5, repeat_rate=-1.0),
               dict(k=5, window=5, repeat_rate=float("nan"))):
        with pytest.raises(N.GbxError) as e:
            KI.index_host(rs, kw["k"], kw["window"], kw.get("repeat_rate", 10.0))
        assert e.value.code == N.GBX_ERR_ARG
    with pytest.raises(N.GbxError) as e:
        KI.minimizers_host(rs, 5, 65)
    assert e.value.code == N.GBX_ERR_ARG
    bad = K.KmerReadSet(rs.enc, np.array([5], dtype=np.int64), np.array([20], dtype=np.int32))
    for call in (lambda: KI.index_host(bad, 5, 5, 10.0), lambda: KI.minimizers_host(bad, 5, 5)):
        with pytest.raises(N.GbxError) as e:
            call()
        assert e.value.code == N.GBX_ERR_ARG
    # 257 reads of 2^31 - 1 bases: the limit is checked on the lengths, before enc is touched, so no such buffer is needed
    n = 257
    big = K.KmerReadSet(np.zeros(16, dtype=np.uint8), np.zeros(n, dtype=np.int64), np.full(n, (1 << 31) - 1, dtype=np.int32))
    p = KI._params(15, 5, 10.0)
    st = KI.KmerIndexStats()
    off = np.zeros(1, dtype=np.int64)
    rc = KI._lib().gbx_kmer_index_host(C.byref(p), n, N.ptr(big.enc), 1 << 40, N.ptr(big.read_off), N.ptr(big.read_len), C.byref(st), None,
                                       N.ptr(off), 0, None, 0)
    assert rc == N.GBX_ERR_UNSUPPORTED and b"2^40" in KI._lib().gbx_last_error()
