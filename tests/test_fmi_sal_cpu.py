"""CPU tests of the suffix-array lookup's contract: the restated LF walk over the host tables (tests/sal_ref.py) equals an
independently computed suffix array, the samples survive a .bwt.2bit.64 round trip, the mem_chain sampling rule."""
import os
import subprocess

import numpy as np
import pytest

from genomicsbench_amd import fmi as FM
from genomicsbench_amd.datagen import gen_fmi_genome
import sal_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute_sa(g):
    """SA of genome + reverse complement + sentinel by sorting the suffixes themselves (the sentinel sorts first)."""
    text = bytes(np.concatenate([g, 3 - g[::-1]]).astype(np.uint8).tolist())
    return np.array(sorted(range(len(text) + 1), key=lambda i: text[i:]), dtype=np.int64)


def small_genomes():
    rng = np.random.default_rng(11)
    elem = rng.integers(0, 4, 40).astype(np.uint8)
    rep = np.concatenate([elem] * 12 + [rng.integers(0, 4, 17).astype(np.uint8)])
    return [np.array([2], np.uint8), np.array([0, 3], np.uint8), np.array([1, 1, 1], np.uint8), np.zeros(64, np.uint8),
            rng.integers(0, 4, 100).astype(np.uint8), rep, rng.integers(0, 4, 2000).astype(np.uint8),
            gen_fmi_genome(2500, 3)]


@pytest.mark.parametrize("sa_compx", [3, 0])
def test_walk_equals_a_brute_force_suffix_sort(sa_compx):
    for g in small_genomes():
        idx, smp = FM.build_index(g, sa_compx=sa_compx)
        want = brute_sa(g)
        n1 = idx.ref_seq_len
        assert len(want) == n1 and want[0] == n1 - 1
        assert smp.n_sa == FM.FmiSa.n_sa_for(n1, sa_compx)
        got = R.sa_walk(idx, smp, np.arange(n1))                       # every row: row 0, the sentinel row, the last row
        assert np.array_equal(got, want), (len(g), sa_compx)
        assert got[idx.sentinel_index] == 0


def test_walk_equals_suffix_array_on_a_300_kbp_genome():
    g = gen_fmi_genome(300_000, 6001)
    idx, smp = FM.build_index(g, sa_compx=3)
    want = FM.suffix_array(np.concatenate([g, 3 - g[::-1]])).numpy()
    rows = np.arange(idx.ref_seq_len)
    got, steps = R.sa_walk(idx, smp, rows, return_steps=True)
    assert np.array_equal(got, want)
    assert steps[::8].max() == 0 and steps.max() > 8                   # sampled rows take no step; some walks are long
    _, s0 = FM.build_index(g, sa_compx=0)
    assert np.array_equal(s0.values(), want)


def test_samples_survive_the_bwa_mem2_file(tmp_path):
    g = gen_fmi_genome(20_000, 7)
    idx, smp = FM.build_index(g, sa_compx=3)
    full = FM.suffix_array(np.concatenate([g, 3 - g[::-1]])).numpy()
    for cx in (3, 0):
        p = FM.save_bwa_mem2_index(idx, str(tmp_path / ("full%d" % cx)), sa=full, sa_compx=cx)
        back, bs = FM.load_bwa_mem2_index(p, with_sa=True)
        assert bs.sa_compx == cx and np.array_equal(bs.values(), full[::1 << cx][:bs.n_sa] if cx else full)
        assert back.sentinel_index == idx.sentinel_index and np.array_equal(back.cp_occ.view(np.uint8), idx.cp_occ.view(np.uint8))
        assert isinstance(FM.load_bwa_mem2_index(p), FM.FmiIndex)        # without with_sa: as before
    # 40-bit values (the upper byte is a signed int8 in the file: values of 2^39 and above included)
    rng = np.random.default_rng(2)
    v = rng.integers(0, 1 << 40, smp.n_sa, dtype=np.int64)
    v[0] = idx.ref_seq_len - 1
    v[1:4] = [(1 << 40) - 1, 1 << 39, (1 << 32) + 5]
    big = FM.FmiSa(3, (v >> 32).astype(np.uint8).view(np.int8), (v & 0xffffffff).astype(np.uint32))
    p = FM.save_bwa_mem2_index(idx, str(tmp_path / "big"), sa=big)
    _, bs = FM.load_bwa_mem2_index(p, with_sa=True)
    assert np.array_equal(bs.values(), v)


def test_all_zero_samples_are_rejected(tmp_path):
    idx = FM.build_index(gen_fmi_genome(5000, 8))
    p = FM.save_bwa_mem2_index(idx, str(tmp_path / "zero"), sa=None)
    with pytest.raises(ValueError, match="not real"):
        FM.load_bwa_mem2_index(p, with_sa=True)
    assert FM.load_bwa_mem2_index(p).ref_seq_len == idx.ref_seq_len      # the seeding benchmark still reads it


@pytest.mark.parametrize("max_occ", [1, 5, 500])
def test_max_occ_sampling_rule(max_occ):
    cases = {1: [0], max_occ: list(range(max_occ)), max_occ + 1: None, 2 * max_occ - 1: None, 2 * max_occ: None, 7 * max_occ + 3: None}
    for s, want in cases.items():
        rows, off = R.hit_rows([100], [s], max_occ)
        step = s // max_occ if s > max_occ else 1
        exp = [100 + i * step for i in range(min(s, max_occ))] if want is None else [100 + w for w in want]
        assert rows.tolist() == exp and off.tolist() == [0, min(s, max_occ)]
        assert rows.max() < 100 + s
    for mo in (0, -3):
        rows, off = R.hit_rows([7, 20], [3, 2 * max_occ + 1], mo)            # <= 0: every row
        assert rows.tolist() == [7, 8, 9] + list(range(20, 20 + 2 * max_occ + 1)) and off.tolist() == [0, 3, 3 + 2 * max_occ + 1]


def test_depos():
    n = 20                                                                   # genome of 10 bases
    is_rev, f = FM.depos(np.array([0, 9, 10, 19]), n)
    assert is_rev.tolist() == [False, False, True, True] and f.tolist() == [0, 9, 9, 0]


def test_driver_print_sa_needs_samples(tmp_path):
    """--print-sa on an index without samples fails with a clear message (before any device work); the help line keeps its text."""
    from genomicsbench_amd.datagen import gen_fmi_reads
    exe = os.path.join(ROOT, "genomicsbench_amd", "bin", "fmi")
    g = gen_fmi_genome(5000, 9)
    idx = FM.build_index(g)
    FM.save_index(idx, str(tmp_path / "g.gbxfmi"))
    FM.save_bwa_mem2_index(idx, str(tmp_path / "z"), sa=None)
    FM.write_reads(str(tmp_path / "r.fq"), gen_fmi_reads(g, 4, 10))
    for ref, what in ((str(tmp_path / "g.gbxfmi"), "has none"), (str(tmp_path / "z"), "not real")):
        r = subprocess.run([exe, ref, str(tmp_path / "r.fq"), "512", "19", "1", "--print-sa"], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and what in r.stderr, r.stderr
    h = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert "Need five arguments : ref_file query_set batch_size minSeedLen n_threads" in h.stderr and "--print-sa" in h.stderr
