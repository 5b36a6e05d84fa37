"""The calls of tests/dbg_cases.py are what they claim to be, shown on the CPU alone: every case's check holds on the
restatement tests/dbg_ref.py, and the hash and table sizing restated in dbg_cases.py equal the product's
(csrc/dbg_hash.h, the header dbg_kernels.hip includes, built for the host by tests/hostcheck/dbg_hash_check.cpp) on random
k-mers and on every frozen colliding k-mer, so those still collide in the kernel's tables.  tests/test_dbg_edges_gpu.py runs
the same calls on the device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dbg_cases as DC
import dbg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {c.name: c for c in DC.all_cases()}


@pytest.fixture(scope="module")
def hostcheck():
    src = os.path.join(ROOT, "tests", "hostcheck", "dbg_hash_check.cpp")
    out = os.path.join(ROOT, "tests", "hostcheck", "libdbg_hash_check.so")
    hdr = os.path.join(ROOT, "genomicsbench_amd", "csrc", "dbg_hash.h")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", src, "-o", out], check=True)
    L = C.CDLL(out)
    L.hostcheck_dbg_node.argtypes = [C.c_char_p, C.c_int, C.c_int64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.hostcheck_dbg_edge.argtypes = [C.c_int64, C.c_int, C.c_int64, C.POINTER(C.c_uint64)]
    L.hostcheck_dbg_sizes.argtypes = [C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.hostcheck_dbg_nodes.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]
    return L


def _node(L, kmer, nc):
    tag, home = C.c_uint64(), C.c_uint64()
    L.hostcheck_dbg_node(kmer, len(kmer), nc, C.byref(tag), C.byref(home))
    return tag.value, home.value


def test_the_case_names_are_unique():
    assert len(CASES) == len(DC.all_cases())


@pytest.mark.parametrize("name", list(CASES))
def test_claims(name):
    """every case is what it is named for, on the restatement and the restated hash"""
    c = CASES[name]
    c.check(c)


@pytest.mark.parametrize("name", list(CASES))
def test_first_touch_keys_give_the_restatement_s_order(name):
    """the first-touch keys restated in dbg_cases.py (what the finish kernel ranks by) order the nodes as the restatement
    does, and the src numbers lie where the k-mer is"""
    c = CASES[name]
    ref_all = b"".join(w[0] for w in c.wins)
    seq_all = b"".join(r[0] for r in c.reads)
    for w in range(c.n_win if c.n_win < 16 else 2):
        g = c.want()[1][w]
        keys, _ = c.first_keys(w)
        assert [n["kmer"] for n in g] == sorted(keys, key=keys.get)
        assert not keys or max(keys.values()) < 2 * c.occ(w)
        for n, s in zip(g, c.src_numbers(w)):
            assert (ref_all[s:s + c.k] if s >= 0 else seq_all[-1 - s:-1 - s + c.k]) == n["kmer"]


@pytest.mark.parametrize("k", [3, 15, 64])
def test_restated_node_hash_equals_the_header(hostcheck, k):
    rng = np.random.default_rng(900 + k)
    rows = np.ascontiguousarray(rng.integers(0, 256, (4000, k), dtype=np.uint8))
    rows[:2000] = np.frombuffer(b"ACGTN", dtype=np.uint8)[rng.integers(0, 5, (2000, k))]
    for nc in (2, 32, 64, 1 << 19, 1 << 40):
        tag, home = np.zeros(len(rows), dtype=np.uint64), np.zeros(len(rows), dtype=np.uint64)
        hostcheck.hostcheck_dbg_nodes(rows.ctypes.data, len(rows), k, nc, tag.ctypes.data, home.ctypes.data)
        h = DC.node_hash(rows)
        assert np.array_equal(tag, h >> np.uint64(DC.TAG_SHIFT)) and np.array_equal(home, h & np.uint64(nc - 1))
    assert int(tag.max()) < 1 << 23
    # the one-k-mer entry and the list form the cases use
    kms = [r.tobytes() for r in rows[:50]]
    assert [_node(hostcheck, km, 64) for km in kms] == list(zip(*DC.node_tag_home(kms, 64)))


def test_restated_edge_home_equals_the_header(hostcheck):
    rng = np.random.default_rng(901)
    home = C.c_uint64()
    for slot, byte, ec in [(0, 0, 2), (0, 255, 32), ((1 << 40) - 1, 65, 1 << 39)] + [
            (int(rng.integers(0, 1 << 30)), int(rng.integers(0, 256)), 1 << int(rng.integers(1, 31))) for _ in range(3000)]:
        hostcheck.hostcheck_dbg_edge(slot, byte, ec, C.byref(home))
        assert home.value == DC.edge_home(slot, byte, ec), (slot, byte, ec)


def test_restated_sizes_equal_the_header(hostcheck):
    nc, ec = C.c_int64(), C.c_int64()
    for c in list(range(0, 2100)) + [(1 << j) + d for j in range(11, 40) for d in (-1, 0, 1)]:
        hostcheck.hostcheck_dbg_sizes(c, C.byref(nc), C.byref(ec))
        assert (nc.value, ec.value) == DC.sizes(c), c
        assert nc.value >= 2 * c + 1 and ec.value >= c + 1 and (c == 0 or (nc.value < 2 * (2 * c + 1) and ec.value < 2 * (c + 1)))
    # the loads the full_tables cases are built for
    assert [DC.sizes(c) for c in (31, 127, 511)] == [(64, 32), (256, 128), (1024, 512)]


def test_frozen_kmers_still_collide_in_the_product_s_hash(hostcheck):
    """tag and home by the header itself, at the nc of every window the k-mers sit in"""
    assert {km for c in DC.families()["collide"] for km in c.facts["kmers"]} == set(DC.frozen_kmers())
    for c in DC.families()["collide"]:
        nc = c.tables(0)[0]
        got = [_node(hostcheck, km, nc) for km in c.facts["kmers"]]
        assert len(set(got)) == 1 and nc in (32, 64), (c.name, got)
        assert got == list(zip(*DC.node_tag_home(list(c.facts["kmers"]), nc)))
    assert {c.tables(0)[0] for c in DC.families()["collide"]} == {32, 64}


def test_the_searches_find_colliding_kmers():
    """the kept searches do what the frozen literals came from, at a width that takes no time: 12 bits of tag and home"""
    saved = DC.TAG_SHIFT, DC.HOME_BITS
    try:
        DC.TAG_SHIFT, DC.HOME_BITS = 58, 6
        a, b = DC.search_pair(14, DC.ACGT, 1, chunk=1 << 12)
        t = DC.search_triple(2, n=1 << 12)
        for kms in ((a, b), t):
            tag, home = DC.node_tag_home(list(kms), 64)
            assert len(set(kms)) == len(kms) and len(set(tag)) == 1 and len(set(home)) == 1
        assert [j for j in range(15) if a[j] != b[j]] == [14]
    finally:
        DC.TAG_SHIFT, DC.HOME_BITS = saved


def test_a_merged_pair_would_show():
    """what the collision cases are for: a table that took a tag match for equality would merge B into A; the restatement
    of that graph differs from the true one in the stats every case is compared on"""
    c = CASES["collide_last_reads"]
    a, b = c.facts["kmers"]
    merged = [(s.replace(b, a), q, f) for s, q, f in c.reads]
    _, st = R.graph(c.wins[0][0], c.wins[0][1], merged, c.k, c.min_qual)
    assert st["n_nodes"] < c.want()[0][0]["n_nodes"] and st["digest"] != c.want()[0][0]["digest"]
