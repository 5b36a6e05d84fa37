"""abea from raw signal on the device: event detection, scalings and the chain into align(), against the CPU restatement
(tests/abea_events_ref.py) and the align oracle.  Everything is compared as bit patterns."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abea_events_ref as R  # noqa: E402
from genomicsbench_amd import abea_signal as AS  # noqa: E402
from genomicsbench_amd.datagen import gen_abea_raw  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "abea_events.npz")
FIELDS = ("start", "length", "mean", "stdv")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same_events(got_off, got_ev, want_off, want_ev):
    assert np.array_equal(got_off, want_off)
    for f in FIELDS:
        assert np.array_equal(_bits(got_ev[f]), _bits(want_ev[f])), f


@pytest.fixture(scope="module")
def case():
    """320 reads of the generator plus the five longest of a larger draw; both summation paths and the reads without events"""
    ss = gen_abea_raw(320, 7001)
    big = gen_abea_raw(2048, 7002)
    longest = np.argsort(big.n_samples)[-5:]
    both = AS.AbeaSignalSet(np.concatenate([ss.raw, big.take(longest).raw]),
                            np.concatenate([ss.raw_off, ss.raw_off[-1] + big.take(longest).raw_off[1:]]),
                            np.concatenate([ss.range, big.range[longest]]), np.concatenate([ss.digitisation, big.digitisation[longest]]),
                            np.concatenate([ss.offset, big.offset[longest]]),
                            np.concatenate([ss.seq_off, big.seq_off[longest] + ss.seq_arena.size]),
                            np.concatenate([ss.seq_len, big.seq_len[longest]]), np.concatenate([ss.seq_arena, big.seq_arena]), ss.model)
    return both, R.run(both, 16)


def _device(ss):
    import torch
    d = AS.DeviceAbeaSignalSet(ss, torch.device("cuda:0"))
    d.run(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d


def test_events_device_equals_restatement(case):
    ss, want = case
    off, ev, scale, shift, status = _device(ss).results()
    assert ss.n_samples.max() >= 100000
    assert np.count_nonzero(status & AS.EV_INORDER) >= 4 and np.count_nonzero((status & AS.EV_INORDER) == 0) >= 200
    assert np.count_nonzero(status & AS.EV_NONE) >= 3
    assert np.array_equal(status & AS.EV_NONE, want["status"])
    assert not np.any(status & AS.EV_OVERFLOW)
    _same_events(off, ev, want["event_off"], want["events"])


def test_scalings_device_equals_restatement(case):
    ss, want = case
    off, ev, scale, shift, status = _device(ss).results()
    assert np.array_equal(_bits(scale), _bits(want["scale"]))
    assert np.array_equal(_bits(shift), _bits(want["shift"]))


def test_events_host_equals_restatement(case):
    ss, want = case
    off, ev, status = AS.events_host(ss)
    _same_events(off, ev, want["event_off"], want["events"])
    # a capacity that is too small: the needed count comes back
    off2, ev2, _ = AS.events_host(ss, event_cap=None if len(ev) == 0 else len(ev))
    assert len(ev2) == len(ev)


def test_signal_align_host_equals_oracle(case):
    from oracle import oracle_py as O
    ss, want = case
    rs, keep = ss.read_set(want["event_off"], want["events"]["mean"], want["scale"], want["shift"])
    wo, wn = O.abea_oracle(rs, 16)
    # not vacuous: under restatement + oracle at least 9 reads in 10 of the whole set align
    assert np.count_nonzero(wn > 0) * 10 >= 9 * ss.n_reads, (np.count_nonzero(wn > 0), ss.n_reads)
    got = AS.signal_align_host(ss)
    _same_events(got["event_off"], got["events"], want["event_off"], want["events"])
    assert np.array_equal(_bits(got["scale"]), _bits(want["scale"])) and np.array_equal(_bits(got["shift"]), _bits(want["shift"]))
    want_np = np.zeros(ss.n_reads, np.int32)
    want_np[keep] = wn
    assert np.array_equal(got["n_pairs"], want_np)
    wp = rs.split_pairs(wo, wn)
    for k, r in enumerate(keep):
        a = 2 * int(got["event_off"][r])
        assert np.array_equal(got["pairs"][a:a + int(wn[k])], wp[k]), r
    # the device objects chain the same way
    import torch
    d = _device(ss)
    drs, dkeep = d.align_set()
    drs.run(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    do, dn = drs.results()
    assert np.array_equal(dkeep, keep) and np.array_equal(dn, wn)


def test_golden_through_device():
    g = np.load(GOLDEN)
    ss = AS.AbeaSignalSet(g["raw"], g["raw_off"], g["range"], g["digitisation"], g["offset"], g["seq_off"], g["seq_len"], g["seq_arena"],
                          g["model"].view(AS.MODEL_DTYPE).reshape(-1))
    off, ev, scale, shift, status = _device(ss).results()
    assert np.array_equal(off, g["event_off"])
    for f in FIELDS:
        assert np.array_equal(_bits(ev[f]), _bits(g["ev_" + f])), f
    assert np.array_equal(_bits(scale), _bits(g["scale"])) and np.array_equal(_bits(shift), _bits(g["shift"]))


def test_empty_call():
    ss = AS.AbeaSignalSet(np.zeros(0, np.int16), np.zeros(1, np.int64), np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.float32),
                          np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros(8, np.uint8), np.zeros(4096, AS.MODEL_DTYPE))
    off, ev, status = AS.events_host(ss)
    assert len(ev) == 0 and off.tolist() == [0]
    got = AS.signal_align_host(ss)
    assert len(got["n_pairs"]) == 0
    from genomicsbench_amd import _native as N
    assert N.lib().gbx_abea_events_device(3, 0, None, None, None, None, None, None, None, None, None, 0, None, None) == 0
    assert N.lib().gbx_abea_scalings_device(0, None, None, None, None, None, None, None, None, None) == 0
