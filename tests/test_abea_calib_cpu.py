"""abea calibration and event-alignment record on the CPU: the restatement (tests/abea_calib_ref.c) against the reference's own
results, the host checks of the entries, the exported symbols, the no-device behaviour and the generator draw the GPU tests use.

tests/golden/abea_calib.npz: six reads (two generated ones of 2 241 and 2 939 bases, one of them with a base outside ACGT; one
with 145 M states; one whose events were moved 8 pA after the alignment, var 4.08; one with six events per k-mer,
events_per_base 6.0; one that align() rejects) with the pairs of align(), and what the reference's own postalign and
recalibrate_model (align.c, compiled unmodified as C++ against empty stand-ins for the htslib / HDF5 headers and called in the
order of scaling_single, f5c.c:1262-1330) made of them: map, events_per_base, both counts, scale, shift, var, log_var, flags.
tests/golden/abea_meth.npz holds the record the reference's get_event_alignment_record returned for five CIGARs and maps."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abea_calib_ref as R  # noqa: E402
from genomicsbench_amd import _native as N  # noqa: E402
from genomicsbench_amd import abea_calib as AC  # noqa: E402
from genomicsbench_amd.abea import AbeaReadSet, MODEL_DTYPE, PAIR_DTYPE  # noqa: E402
from genomicsbench_amd.datagen import bam_cigar, gen_abea_cigars, gen_abea_raw  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SEED, FIRST = 8201, 8                                    # the one call's draw: reads 8 .. 15 of seed 8201


def golden_calib():
    """-> (AbeaReadSet, pairs in the 2 x event_off layout, n_pairs, the npz)"""
    g = np.load(os.path.join(HERE, "golden", "abea_calib.npz"))
    rs = AbeaReadSet(g["seq_off"], g["seq_len"], g["seq_arena"], g["event_off"], g["event_mean"], g["scale_in"], g["shift_in"],
                     np.ascontiguousarray(g["model"]).view(MODEL_DTYPE).reshape(-1))
    pairs, o = np.zeros(2 * int(rs.event_off[-1]), PAIR_DTYPE), 0
    for r in range(rs.n_reads):
        k = int(g["n_pairs"][r])
        pairs[2 * int(rs.event_off[r]):2 * int(rs.event_off[r]) + k] = np.ascontiguousarray(g["pairs"][o:o + k]).view(PAIR_DTYPE).reshape(-1)
        o += k
    return rs, pairs, g["n_pairs"], g


def assert_calib_equals_golden(c, rs, g):
    assert np.array_equal(R.read_maps(c["map"], rs.seq_off, rs.seq_len), g["map"])
    for k in ("scale", "shift", "var", "log_var"):
        assert np.array_equal(np.ascontiguousarray(c[k][:rs.n_reads]).view(np.uint32), g[k]), k
    for k in ("events_per_base", "n_event_alignment", "n_m_state", "flags"):
        assert np.array_equal(c[k][:rs.n_reads], g[k]), k


def test_restatement_equals_reference():
    rs, pairs, n_pairs, g = golden_calib()
    assert g["flags"].tolist() == [0, 0, 1, 1, 4, 2] and g["n_m_state"][2] < 200 <= g["n_m_state"][3]
    c = R.calibrate(rs.seq_off, rs.seq_len, rs.seq_arena, rs.event_off, rs.event_mean, rs.model, pairs, n_pairs, rs.scale, rs.shift)
    assert_calib_equals_golden(c, rs, g)
    assert np.array_equal(c["log_var"][:2], np.log(c["var64"][:2]).astype(np.float32))


def golden_record_inputs():
    g = np.load(os.path.join(HERE, "golden", "abea_meth.npz"))
    # the file keeps a read's n_kmers entries back to back; the entries index the map like an arena of bases, 5 slots more
    m = np.concatenate([g["base_to_event_map"], np.full((8, 2), -9, np.int32)])
    return g, (g["cigar_off"], g["cigar"], g["ref_start_pos"], g["rc"], g["map_off"][:-1], g["read_len"], m)


def test_record_restatement_equals_reference():
    g, args = golden_record_inputs()
    rec_off, rec = R.record(*args)
    assert np.array_equal(rec_off, g["rec_off"]) and np.array_equal(rec.view(np.int32).reshape(-1, 2), g["rec"])


def test_record_restatement_refuses_what_the_reference_refuses():
    m = np.zeros((40, 2), np.int32)
    for ops in ([(40, "N")], [(3, "P")], [(41, "M")]):
        with pytest.raises(ValueError):
            R.record([0, 1], bam_cigar(ops), [0], [0], [0], [40], m)
    with pytest.raises(ValueError):
        R.record([0, 1], np.array([5 << 4 | 9], np.uint32), [0], [0], [0], [40], m)


def test_symbols_exported():
    L = N.lib()
    for f in ("gbx_abea_calib_device", "gbx_abea_calib_host", "gbx_abea_calib_logvar_host", "gbx_abea_event_record_device",
              "gbx_abea_event_record_host", "gbx_abea_call_methylation_host"):
        assert hasattr(L, f), f


def test_logvar_host_is_the_double_logarithm():
    v = np.array([1.0332748889923096, 4.0771, 0.3, 2.0])
    got = AC.logvar_host(v, [200, 5000, 199, 0])
    assert np.array_equal(got.view(np.uint32), np.array([np.log(v[0]), np.log(v[1]), 0, 0]).astype(np.float32).view(np.uint32))


def test_calib_host_refuses_pairs_that_decrease():
    rs, pairs, n_pairs, _ = golden_calib()
    for field in ("ref_pos", "read_pos"):
        bad = pairs.copy()
        at = 2 * int(rs.event_off[1]) + 100
        bad[field][at] = bad[field][at - 1] - 1
        with pytest.raises(N.GbxError) as e:
            AC.calibrate_host(rs, bad, n_pairs)
        assert e.value.code == N.GBX_ERR_ARG and "read 1" in str(e.value) and "pair 100" in str(e.value)
    bad = pairs.copy()
    bad["read_pos"][2 * int(rs.event_off[3]) + int(n_pairs[3]) - 1] = rs.n_events[3]          # past the read's events
    with pytest.raises(N.GbxError) as e:
        AC.calibrate_host(rs, bad, n_pairs)
    assert e.value.code == N.GBX_ERR_ARG and "read 3" in str(e.value)


def test_record_host_refuses_what_the_reference_refuses():
    m = np.zeros((40, 2), np.int32)
    cases = [bam_cigar([(10, "M"), (5, "N"), (10, "M")]), bam_cigar([(3, "P")]), np.array([5 << 4 | 9], np.uint32), bam_cigar([(20, "="), (21, "X")])]
    for cig in cases:
        with pytest.raises(N.GbxError) as e:
            AC.event_record_host([0, len(cig)], cig, [0], [0], [0], [40], m)
        assert e.value.code == N.GBX_ERR_ARG and "read 0" in str(e.value)


def test_entries_need_a_device():
    """No CPU fallback: without a device the entries fail with GBX_ERR_NO_DEVICE."""
    if N.device_count() > 0:
        pytest.skip("a GPU is present")
    rs, pairs, n_pairs, _ = golden_calib()
    with pytest.raises(N.GbxError) as e:
        AC.calibrate_host(rs, pairs, n_pairs)
    assert e.value.code == N.GBX_ERR_NO_DEVICE
    _, args = golden_record_inputs()
    with pytest.raises(N.GbxError) as e:
        AC.event_record_host(*args)
    assert e.value.code == N.GBX_ERR_NO_DEVICE
    ss = gen_abea_raw(2, SEED, FIRST)
    with pytest.raises(N.GbxError) as e:
        AC.call_methylation_host(ss, gen_abea_cigars(ss, SEED, FIRST))
    assert e.value.code == N.GBX_ERR_NO_DEVICE
    L = AC._lib()
    one = np.zeros(8, np.int64)
    p = N.ptr(one)
    assert L.gbx_abea_calib_device(1, *([p] * 17), None) == N.GBX_ERR_NO_DEVICE
    assert L.gbx_abea_event_record_device(1, 1, *([p] * 11), 0, None) == N.GBX_ERR_NO_DEVICE


def test_empty_batches_return_ok():
    L = AC._lib()
    assert L.gbx_abea_calib_device(0, *([None] * 18)) == 0 and L.gbx_abea_event_record_device(3, 0, *([None] * 11), 0, None) == 0
    assert L.gbx_abea_calib_host(0, None, None, None, 0, *([None] * 15)) == 0
    n = np.zeros(1, np.int64)
    assert L.gbx_abea_event_record_host(0, *([None] * 6), 0, None, None, None, 0, None, N.ptr(n)) == 0
    assert L.gbx_abea_call_methylation_host(0, *([None] * 8), 0, *([None] * 15), 0, None, None, N.ptr(n)) == 0


def test_generator_draw():
    """The draw of the one-call GPU test, on the restatements: every CIGAR operation, both strands, the reference segment
    consistent with the CIGAR, at least 4 unflagged reads with at least 100 sites between them and at least one flagged read."""
    ss = gen_abea_raw(8, SEED, FIRST)
    cg, again = gen_abea_cigars(ss, SEED, FIRST), gen_abea_cigars(ss, SEED, FIRST)
    assert all(np.array_equal(cg[k], again[k]) for k in cg)
    ops = set((cg["cigar"] & 0xf).tolist())
    assert ops == {0, 1, 2, 4, 5, 7, 8} and set(cg["rc"].tolist()) == {0, 1}
    for r in range(8):
        c = cg["cigar"][cg["cigar_off"][r]:cg["cigar_off"][r + 1]]
        ln, op = (c >> 4).astype(np.int64), c & 0xf
        assert ln[np.isin(op, (0, 1, 4, 7, 8))].sum() == ss.seq_len[r] and ln[np.isin(op, (0, 2, 7, 8))].sum() == cg["ref_len"][r]
    w = R.call_methylation(ss, cg, 16)
    ok = w["flags"] == 0
    assert ok.sum() >= 4 and (~ok).sum() >= 1 and len(w["sites"]) >= 100
    assert set(np.unique(w["sites"]["read"]).tolist()) <= set(np.flatnonzero(ok).tolist())
    assert np.all(np.diff(w["rec_off"])[~ok] == 0)
