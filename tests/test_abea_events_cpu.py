"""abea from raw signal, the parts that need no GPU: the CPU restatement (tests/abea_events_ref.c) against tables the
reference produced, hand-checkable signals, the generator, the exported symbols and the no-device behaviour.

tests/golden/abea_events.npz: five generated reads (two short ones, one with a low-amplitude stretch, one with negative pA,
one of 100 006 samples) with the event tables and scalings that the reference's own events.c (getevents) and
estimate_scalings_using_mom (align.c:49-97) gave for them, compiled unmodified with empty stand-ins for the htslib / HDF5
headers and driven as event_single (f5c.c:1219-1242) does.  Only the data is kept."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abea_events_ref as R  # noqa: E402
from genomicsbench_amd import _native as N  # noqa: E402
from genomicsbench_amd import abea_signal as AS  # noqa: E402
from genomicsbench_amd.datagen import gen_abea, gen_abea_raw  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "abea_events.npz")
RG, DG = np.float32(1467.61), np.float32(8192.0)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _one(adc, offset=0.0):
    adc = np.asarray(adc, np.int16)
    return R.detect(adc, np.array([0, len(adc)], np.int64), [RG], [DG], [np.float32(offset)], 1)


def test_restatement_equals_reference_tables():
    g = np.load(GOLDEN)
    assert np.diff(g["raw_off"]).max() >= 100000
    ss = AS.AbeaSignalSet(g["raw"], g["raw_off"], g["range"], g["digitisation"], g["offset"], g["seq_off"], g["seq_len"], g["seq_arena"],
                          g["model"].view(AS.MODEL_DTYPE).reshape(-1))
    got = R.run(ss, 4)
    assert np.array_equal(got["event_off"], g["event_off"])
    for f in ("start", "length", "mean", "stdv"):
        assert np.array_equal(_bits(got["events"][f]), _bits(g["ev_" + f])), f
    assert np.array_equal(_bits(got["shift"]), _bits(g["shift"]))
    assert np.array_equal(_bits(got["scale"]), _bits(g["scale"]))


def test_staircase_boundaries():
    """Noise-free steps every 20 samples: within a level both windows have zero variance, so the t-statistic is largest
    exactly where the windows lie on either side of a step; the events are the levels."""
    levels = np.array([400, 520, 450, 610, 380, 500, 560, 430], np.int16)
    adc = np.repeat(levels, 20)
    off, ev, st = _one(adc)
    assert st.tolist() == [0]
    assert ev["start"].tolist() == list(range(0, 160, 20))
    assert ev["length"].tolist() == [20.0] * 8
    want = (levels.astype(np.float32) + np.float32(0)) * (RG / DG)
    assert np.allclose(ev["mean"], want, rtol=1e-6) and np.all(ev["stdv"] < 0.05)


def test_reads_without_events():
    for adc in (np.zeros(0, np.int16), np.arange(500, 505, dtype=np.int16), np.full(500, 512, np.int16)):
        off, ev, st = _one(adc)
        assert off.tolist() == [0, 0] and len(ev) == 0 and st.tolist() == [1]


def test_generator_is_deterministic_and_has_edge_reads():
    a, b = gen_abea_raw(192, 7001), gen_abea_raw(192, 7001)
    for f in ("raw", "raw_off", "range", "digitisation", "offset", "seq_arena", "seq_len"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    c = gen_abea_raw(16, 7001, first=40)                 # a sub-range regenerates the same reads
    assert np.array_equal(c.raw, a.raw[a.raw_off[40]:a.raw_off[56]])
    assert not np.array_equal(gen_abea_raw(4, 7002).raw[:1000], a.raw[:1000])
    rs = gen_abea(192, 7001)                             # the reads are gen_abea's
    assert np.array_equal(rs.seq_len, a.seq_len) and np.array_equal(rs.scale, a.true_scale)
    ns = a.n_samples
    assert ns[47] == 0 and ns[111] == 5 and ns[175] == 500
    pa = lambda r: (a.raw[a.raw_off[r]:a.raw_off[r + 1]].astype(np.float32) + a.offset[r]) * (a.range[r] / a.digitisation[r])
    assert pa(29).min() < 0 < pa(29).max()               # negative pA
    assert np.abs(pa(13)[1000:1300]).max() < 4 and np.abs(pa(13)[2000:]).min() > 20      # a low-amplitude stretch
    dwell = ns[0] / (a.seq_len[0] - 5)
    assert 7.5 < dwell < 10.5
    want = R.run(a, 4)
    assert np.array_equal(np.flatnonzero(want["status"]), [47, 111, 175])


def test_symbols_exported():
    L = N.lib()
    for f in ("gbx_abea_events_device", "gbx_abea_scalings_device", "gbx_abea_events_host", "gbx_abea_signal_align_host"):
        assert hasattr(L, f), f


def test_argument_errors_come_first():
    ss = gen_abea_raw(3, 7001)
    ss.raw_off = ss.raw_off.copy(); ss.raw_off[1] = ss.raw_off[2] + 5
    with pytest.raises(N.GbxError) as e:
        AS.events_host(ss)
    assert e.value.code == N.GBX_ERR_ARG
    ss = gen_abea_raw(3, 7001)
    ss.seq_len = ss.seq_len.copy(); ss.seq_len[1] = 3
    with pytest.raises(N.GbxError) as e:
        AS.signal_align_host(ss)
    assert e.value.code == N.GBX_ERR_ARG


def test_host_entries_need_a_device():
    """No CPU fallback: without a device the host entries fail with GBX_ERR_NO_DEVICE."""
    if N.device_count() > 0:
        pytest.skip("a GPU is present")
    ss = gen_abea_raw(3, 7001)
    for fn in (AS.events_host, AS.signal_align_host):
        with pytest.raises(N.GbxError) as e:
            fn(ss)
        assert e.value.code == N.GBX_ERR_NO_DEVICE
