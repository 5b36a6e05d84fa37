"""The calls of tests/kmer_cases.py are what they claim to be, shown on the CPU alone: for every case the restatement
tests/kmer_ref.py counts exactly the case's own expectation (a dict code -> count, from which stats, histogram and selection
follow), the laid-out cases agree with a third formulation over text k-mers, every entry of a case's `facts` holds, and the
unit size, sweep split and slice rule restated in kmer_cases.py equal the product's (csrc/kmer_split.h, the header
kmer_kernels.hip includes, built for the host by tests/hostcheck/kmer_split_check.cpp).  tests/test_kmer_edges_gpu.py runs
the same calls on the device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kmer_cases as KC
import kmer_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {c.name: c for c in KC.all_cases()}


@pytest.fixture(scope="module")
def hostcheck():
    src = os.path.join(ROOT, "tests", "hostcheck", "kmer_split_check.cpp")
    out = os.path.join(ROOT, "tests", "hostcheck", "libkmer_split_check.so")
    hdr = os.path.join(ROOT, "genomicsbench_amd", "csrc", "kmer_split.h")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", src, "-o", out], check=True)
    L = C.CDLL(out)
    L.hostcheck_kmer_constants.argtypes = [C.POINTER(C.c_int64)]
    L.hostcheck_kmer_sweep_split.argtypes = [C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.hostcheck_kmer_slices.argtypes = [C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.hostcheck_kmer_read_units.argtypes = [C.c_int64, C.c_int]
    L.hostcheck_kmer_read_units.restype = C.c_int64
    L.hostcheck_kmer_sweep_splits.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def ref():
    """name -> kmer_ref.count_ref of the case, computed once per set of reads and parameters"""
    memo = {}

    def get(name):
        c = CASES[name]
        key = (id(c.reads), c.k, c.n_hist, c.min_freq, c.max_freq)
        if key not in memo:
            memo[key] = R.count_ref(c.reads, c.k, **c.params())
        return memo[key]
    return get


def same(got, want):
    assert got[0] == want[0]
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    assert got[2].dtype == want[2].dtype == np.uint64 and got[3].dtype == want[3].dtype == np.uint32


def test_the_case_names_are_unique():
    assert len(CASES) == len(KC.all_cases())
    assert set(KC.families()) == {"chunk_word", "high_bits", "strands", "units", "sweep", "select", "slices"}
    assert all(c.family == fam for fam, cs in KC.families().items() for c in cs)


@pytest.mark.parametrize("name", list(CASES))
def test_the_restatement_counts_the_expectation(name, ref):
    c = CASES[name]
    same(ref(name), c.want())
    assert all(KC.is_canonical(code, c.k) and n > 0 for code, n in c.table.items())
    assert 0 <= c.sel_cap and c.need == len(c.want()[2])


@pytest.mark.parametrize("name", [c.name for c in KC.all_cases() if c.seqs is not None])
def test_laid_out_reads_by_text(name, ref):
    """a third formulation, from the bytes of enc: text windows, canonical by string reversal and complement"""
    c = CASES[name]
    texts = KC.read_texts(c.reads)
    assert texts == c.seqs
    same(ref(name), KC.expect(KC.text_table(texts, c.k), c.n_hist, c.min_freq, c.max_freq))


def test_planted_refuses_what_is_not_canonical():
    assert not KC.is_canonical(KC.code_of("TTA"), 3)
    for bad in ({KC.code_of("TTA"): 1}, {64: 1}, {0: 0}, {-1: 2}):
        with pytest.raises(ValueError):
            KC.planted(3, bad)
    rs = KC.planted(3, {KC.code_of("ACG"): 3, KC.code_of("AAT"): 2})
    assert rs.read_len.tolist() == [4] * 5
    first = ["".join("ACGT"[b] for b in rs.enc[o:o + 3]) for o in rs.read_off.tolist()]
    assert first == ["AAT", "ATT", "ACG", "CGT", "ACG"]                                # the strands alternate
    assert len(set(rs.enc[3::4].tolist())) > 1                                          # the base no window holds varies


# ------------------------------------------------------------------------------------------------- the facts
def count_of(res_table, code):
    return res_table.get(code, 0)


def ref_table(c):
    codes, counts = np.unique(R.canonical_codes(c.reads, c.k), return_counts=True)
    return dict(zip(codes.tolist(), counts.tolist()))


def check_split(c, v, t):
    assert KC.sweep_split(KC.slice_rule(c.k)[0]) == tuple(v)


def check_pairs(c, v, t):
    whats = set()
    for what, unit, b, lo, hi in v:
        assert lo < b <= hi and b % unit == 0
        assert lo // unit == b // unit - 1 and hi // unit == b // unit, (what, b, lo, hi)       # still the neighbouring shares
        assert t.get(lo, 0) > 0 and t.get(hi, 0) > 0, (what, lo, hi)
        assert not KC.canonical_codes(c.k, lo + 1, b) and not KC.canonical_codes(c.k, b, hi)     # the nearest canonical ones
        whats.add(what)
    slice_n = KC.slice_rule(c.k)[0]
    nb, per = KC.sweep_split(slice_n)
    assert whats == {w for w, n in (("lane", KC.LANE), ("wave", KC.WAVE), ("round", KC.KC_SWEEP), ("workgroup", per), ("scan", KC.SCAN_TRIP * per))
                     if n < slice_n}
    if c.k == 11:
        assert nb > KC.SCAN_TRIP and ("lane", 4, 24, 23, 24) in [tuple(p) for p in v]          # indices 4t + 3 and 4t + 4 themselves
    lane = [p for p in v if p[0] == "lane"]
    if lane:
        assert sum(t.get(x, 0) > 0 for x in range(lane[0][4], lane[0][4] + KC.LANE)) >= 2       # two counters of one lane


def check_last_canonical(c, v, t):
    assert KC.is_canonical(v, c.k) and not KC.canonical_codes(c.k, max(v + 1, 4 ** c.k - (1 << 20)), 4 ** c.k) and t[v] > 0
    if c.k % 2 == 0 and c.k > 1:
        assert v == KC.revcomp(v, c.k) == KC.code_of("T" * (c.k // 2) + "A" * (c.k // 2))
    if c.k == 17:
        assert v == KC.code_of("T" * 8 + "C" + "A" * 8) and v // KC.KC_SLICE == 15


def check_bins(c, v, t):
    n = c.n_hist
    assert v == [x for x in (n - 2, n - 1, n, n + 5) if x > 0] and all(x in t.values() for x in v)
    assert set(KC.COUNTS) <= set(t.values())


def check_cut(c, v, t):
    kind, c1, c2 = v
    sel = [int(x) for x in c.want()[2]]
    cap = c.sel_cap
    assert 0 < cap < len(sel) and (sel[cap - 1], sel[cap]) == (c1, c2)
    assert KC.cut_kind(c1, c2, c.k) == kind
    slice_n = KC.slice_rule(c.k)[0]
    per = KC.sweep_split(slice_n)[1]
    i1, i2 = c1 % slice_n, c2 % slice_n
    same_slice = c1 // slice_n == c2 // slice_n
    if kind == "lane":
        assert same_slice and i1 // 4 == i2 // 4
    elif kind == "wave":
        assert same_slice and i1 // 256 + 1 == i2 // 256 and i1 // 1024 == i2 // 1024
    elif kind == "round":
        assert same_slice and i1 // 1024 + 1 == i2 // 1024 and i1 // per == i2 // per
    elif kind == "workgroup":
        assert same_slice and i1 // per < i2 // per
    else:
        assert kind == "slice" and c1 // slice_n < c2 // slice_n
    # a later workgroup whose first output slot is at or behind sel_cap: it leaves at once
    wgs = [KC.workgroup_of(x, c.k) for x in sel]
    assert any(w > wgs[cap - 1] and wgs.index(w) >= cap for w in wgs)


def check_need(c, v, t):
    assert v == c.need > 2


def check_workgroups(c, v, t):
    sel = [int(x) for x in c.want()[2]]
    assert sorted({KC.workgroup_of(x, c.k) for x in sel}) == list(v) and len(sel) >= len(v)
    others = {KC.workgroup_of(x, c.k) for x in t} - set(v)
    assert others                                                          # counters that are not selected lie elsewhere
    if len(v) == 1:
        per = KC.sweep_split(KC.slice_rule(c.k)[0])[1]
        assert per > KC.KC_SWEEP and {x % per // KC.KC_SWEEP for x in sel} == set(range(per // KC.KC_SWEEP))      # in every round of it
    else:
        assert [b - a for a, b in zip(v, v[1:])] == [64] * (len(v) - 1) and v[0] == 0 and v[-1] > KC.SCAN_TRIP


def check_slices_selected(c, v, t):
    slice_n, n_slices = KC.slice_rule(c.k)
    sel = [int(x) for x in c.want()[2]]
    assert [sum(x // slice_n == s for x in sel) for s in range(n_slices)] == list(v)
    if c.k == 16:
        assert v[2] == 0 and any(x // slice_n == 2 for x in t) and v[0] and v[1] >= 2 and v[3]


def check_slices_held(c, v, t):
    assert sorted({x // KC.slice_rule(c.k)[0] for x in t}) == list(v)


def check_borders(c, v, t):
    slice_n, n_slices = KC.slice_rule(c.k)
    assert [b for b, _, _ in v] == [j * slice_n for j in range(1, n_slices)] and n_slices == 4
    for b, lo, hi in v:
        assert lo < b <= hi and t.get(lo, 0) > 0 and t.get(hi, 0) > 0
        assert not KC.canonical_codes(c.k, lo + 1, b) and not KC.canonical_codes(c.k, b, hi)
        nb, per = KC.sweep_split(slice_n)
        assert lo % slice_n // per == nb - 1 and hi % slice_n // per == 0           # the last and the first workgroup of their slices


def check_top_text(c, v, t):
    assert t.get(KC.code_of(v), 0) > 0 and KC.code_of(v) // KC.slice_rule(c.k)[0] == 3


def check_residues(c, v, t):
    off, ln = c.reads.read_off, c.reads.read_len.astype(np.int64)
    assert set(v) == set(KC.DELTAS) == {1, 2, 255, 256, 257, 511, 512, 513}
    for d, want in v.items():
        assert sorted((off[ln - c.k == d] % 16).tolist()) == list(want) == list(range(16))
    assert {KC.read_units(int(n), c.k) for n in ln} == {1, 2, 3}


def check_fill(c, v, t):
    owned = np.zeros(c.reads.enc.size, dtype=bool)
    for o, n in zip(c.reads.read_off.tolist(), c.reads.read_len.tolist()):
        owned[o:o + n] = True
    gaps = c.reads.enc[~owned] & 3
    if "junk_of" in c.facts:
        return
    assert gaps.size > 0
    assert {"zeros": not gaps.any(), "hostile": gaps.all(), "mixed": gaps.any() and not gaps.all()}[v]
    # a gap byte lies right in front of a read and right behind one: inside the first and the last word the count pass loads
    starts, ends = c.reads.read_off, c.reads.read_off + c.reads.read_len
    assert (~owned[starts[starts > 0] - 1]).any() and (~owned[ends[ends < owned.size]]).any()


def check_one_word(c, v, t):
    for r in v:
        o, n = int(c.reads.read_off[r]), int(c.reads.read_len[r])
        assert n > c.k and o // 16 == (o + n - 1) // 16
    assert any(int(c.reads.read_off[r]) % 16 and (int(c.reads.read_off[r]) + int(c.reads.read_len[r])) % 16 for r in v)


def check_enc_end(c, v, t):
    o, n = int(c.reads.read_off[-1]), int(c.reads.read_len[-1])
    assert o + n == c.reads.enc.size and c.reads.enc.size % 16 != 0 and n > c.k


def check_overlap(c, v, t):
    off, ln = c.reads.read_off.tolist(), c.reads.read_len.tolist()
    for a, b in v:
        assert max(off[a], off[b]) < min(off[a] + ln[a], off[b] + ln[b])
    assert sum(ln) > c.reads.enc.size


def check_junk_of(c, v, t):
    base = CASES[v]
    assert np.array_equal(c.reads.enc & 3, base.reads.enc) and base.reads.enc.max() <= 3
    assert (c.reads.enc >> 2).max() == 63 and c.table == base.table
    last = c.reads.enc[(c.reads.read_off + c.reads.read_len - 1)[c.reads.read_len > 0]]
    assert (last > 3).any()                                                 # the base no window holds, too


def check_palindromes(c, v, t):
    assert len(v) >= 4 and {0, 1} == set(v.values())
    for code, parity in v.items():
        assert KC.revcomp(code, c.k) == code and t[code] & 1 == parity
    twin = CASES[c.name[:-1] + ("b" if c.name.endswith("a") else "a")]
    assert all(twin.facts["palindromes"][code] != parity for code, parity in v.items())          # odd here, even there


def check_reverse_only(c, v, t):
    assert len(v) >= 2
    firsts = set()
    for o, n in zip(c.reads.read_off.tolist(), c.reads.read_len.tolist()):
        firsts.add(int("".join(str(b) for b in c.reads.enc[o:o + c.k].tolist()), 4))
    for code in v:
        assert t[code] > 0 and code not in firsts and KC.revcomp(code, c.k) in firsts and KC.revcomp(code, c.k) > code


def check_homopolymers(c, v, t):
    a, b = (c.reads.enc[int(c.reads.read_off[r]):int(c.reads.read_off[r]) + int(c.reads.read_len[r])] for r in v)
    assert a.size > c.k + 1 and b.size > c.k + 1 and not a.any() and (b == 3).all()
    assert t[0] == a.size - c.k + b.size - c.k


def check_units(c, v, t):
    f = c.facts
    ln = c.reads.read_len.tolist()
    units = [KC.read_units(n, c.k) for n in ln]
    assert len(ln) == f["n_reads"] and KC.unit_share(len(ln)) == f["share"] == -(-len(ln) // 1024)
    if len(ln) == 1:
        assert units == [1]
        return
    assert ln[0] == 0 and ln[-1] == c.k and units[0] == units[-1] == 0
    start, length = f["run"]
    assert length > f["share"] and not any(units[start:start + length]) and units[start - 1] and units[start + length]
    assert {ln[i] for i in range(start, start + length)} == {0, c.k - 1, c.k}
    for i in f["singles"]:
        assert units[i] == 0 and units[i - 1] and units[i + 1]
    assert units[f["long"]] == 3 and sorted(set(units)) == [0, 1, 3] and units.count(3) == 1
    # reads that have units on both sides of a thread's share, and a thread whose whole share is unit-less
    share = f["share"]
    assert any(units[i - 1] and units[i] for i in range(share, len(ln), share))
    assert any(not any(units[i:i + share]) for i in range(share, len(ln) - share, share))


CHECKS = dict(split=check_split, pairs=check_pairs, last_canonical=check_last_canonical, bins=check_bins, cut=check_cut, need=check_need,
              workgroups=check_workgroups, slices_selected=check_slices_selected, slices_held=check_slices_held, borders=check_borders,
              top_text=check_top_text, residues=check_residues, fill=check_fill, one_word=check_one_word, enc_end=check_enc_end,
              overlap=check_overlap, junk_of=check_junk_of, palindromes=check_palindromes, reverse_only=check_reverse_only,
              homopolymers=check_homopolymers, n_reads=check_units)
UNITS_PARTS = ("share", "run", "singles", "long")                         # checked with n_reads


@pytest.mark.parametrize("name", list(CASES))
def test_facts(name):
    """every case is what it is named for, on the restatement and the restated split"""
    c = CASES[name]
    t = ref_table(c)
    assert c.facts, name
    for fact, v in c.facts.items():
        if fact not in UNITS_PARTS:
            CHECKS[fact](c, v, t)


def test_the_families_hold_what_the_kernels_branch_on():
    fam = KC.families()
    assert sorted({c.k for c in fam["chunk_word"] if "residues" in c.facts}) == [1, 2, 9, 16, 17]
    assert {c.facts["fill"] for c in fam["chunk_word"]} == {"zeros", "hostile", "mixed"}
    assert all(any(key in c.facts for c in fam["chunk_word"]) for key in ("one_word", "enc_end", "overlap"))
    assert sorted({c.k for c in fam["strands"]}) == [2, 10, 16]
    assert sorted(c.facts["n_reads"] for c in fam["units"]) == [1, 1023, 1024, 1025, 2049, 3000]
    assert sorted({c.k for c in fam["sweep"]}) == [1, 2, 6, 11] and sorted({c.n_hist for c in fam["sweep"]} - {32}) == [2, 3, 17, 4096]
    sel = [c for c in fam["select"] if c.name.startswith("select_min")]
    assert {(c.min_freq, c.max_freq) for c in sel} == {(1, 0), (2, 2), (2, 16), (16, 0), (3, 2), (0, 5), (1, 2 ** 32 - 1)}
    assert {c.need for c in sel if c.min_freq in (0, 3)} == {0}
    caps = [c for c in fam["select"] if c.name.startswith("select_cap")]
    assert sorted(c.sel_cap - c.need for c in caps if c.sel_cap > 1) == [-1, 0, 1] and sorted(c.sel_cap for c in caps)[:2] == [0, 1]
    assert {c.facts["cut"][0] for c in fam["select"] if "cut" in c.facts} == {"lane", "wave", "round", "workgroup"}
    assert {c.facts["cut"][0] for c in fam["slices"] if "cut" in c.facts} == {"workgroup", "slice"}
    assert len([c for c in KC.all_cases() if c.k >= 15]) <= 12                # each call clears and sweeps 4 GB per slice
    assert {c.family for c in KC.all_cases() if c.reads.enc.size and c.reads.enc.max() > 3} == {"high_bits"}


# ------------------------------------------------------------------------------------------------- the split against the header
def test_restated_constants_equal_the_header(hostcheck):
    out = (C.c_int64 * 5)()
    hostcheck.hostcheck_kmer_constants(out)
    assert list(out) == [KC.KC_CHUNK, KC.KC_THREADS, KC.KC_SWEEP, KC.KC_MAX_BLOCKS, KC.KC_SLICE]
    assert KC.LANE * 64 == KC.WAVE and KC.WAVE * (KC.KC_THREADS // 64) == KC.KC_SWEEP


def test_restated_sweep_split_equals_the_header(hostcheck):
    ns = sorted({m * 1024 + d for m in range(0, (1 << 22) // 1024 + 1) for d in (-1, 0, 1) if m * 1024 + d > 0} |
                {(1 << 30) + d for d in (-1, 0, 1)} | {4 ** k for k in range(1, 16)} | set(range(1, 5000)))
    n = np.array(ns, dtype=np.int64)
    nb, per = np.zeros_like(n), np.zeros_like(n)
    hostcheck.hostcheck_kmer_sweep_splits(n.ctypes.data, n.size, nb.ctypes.data, per.ctypes.data)
    want = [KC.sweep_split(x) for x in ns]
    assert nb.tolist() == [w[0] for w in want] and per.tolist() == [w[1] for w in want]
    assert (per % KC.KC_SWEEP == 0).all() and (nb <= KC.KC_MAX_BLOCKS).all() and (nb * per >= n).all() and ((nb - 1) * per < n).all()
    one_nb, one_per = C.c_int64(), C.c_int64()
    hostcheck.hostcheck_kmer_sweep_split(4 ** 11, C.byref(one_nb), C.byref(one_per))
    assert (one_nb.value, one_per.value) == (2048, 2048) == KC.sweep_split(4 ** 11)


def test_restated_slices_and_units_equal_the_header(hostcheck):
    sn, ns = C.c_int64(), C.c_int64()
    for k in range(1, 18):
        hostcheck.hostcheck_kmer_slices(k, C.byref(sn), C.byref(ns))
        assert (sn.value, ns.value) == KC.slice_rule(k) and sn.value * ns.value == 4 ** k
        for length in range(0, 2001):
            assert hostcheck.hostcheck_kmer_read_units(length, k) == KC.read_units(length, k)
    assert [KC.slice_rule(k)[1] for k in (15, 16, 17)] == [1, 4, 16]
    assert [KC.read_units(9 + d, 9) for d in (-9, 0, 1, 255, 256, 257, 512, 513)] == [0, 0, 1, 1, 1, 2, 2, 3]
