"""abea eventalign on the device and through the host entries, against the CPU restatement (tests/abea_eventalign_ref.py, and those
of the stages in front of it) and the reference's own results (tests/golden/abea_eventalign.npz).  Records, statuses and summary
fields are compared as bit patterns, the TSV as bytes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abea_eventalign_ref as R  # noqa: E402
from genomicsbench_amd import _native as N  # noqa: E402
from genomicsbench_amd import abea_calib as AC  # noqa: E402
from genomicsbench_amd import abea_eventalign as EA  # noqa: E402
from genomicsbench_amd.datagen import gen_abea_cigars, gen_abea_raw  # noqa: E402
from test_abea_calib_cpu import FIRST, SEED  # noqa: E402
from test_abea_eventalign_cpu import assert_records_equal_golden, golden, golden_groups, subset  # noqa: E402

pytestmark = pytest.mark.gpu


def _device_eventalign(seq_off, seq_len, event_off, event_mean, model, calib, cg, region=(-1, -1), rows_cap=EA.ROWS_CAP, order=True):
    """the count pass of gbx_abea_event_record_device (the near table), then gbx_abea_eventalign_device, on torch tensors"""
    import torch
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    n = len(seq_len)
    total = int(event_off[n])
    cig = np.ascontiguousarray(cg["cigar"], np.uint32)
    n_cig = int(cg["cigar_off"][n])
    d = dict(seq_off=t(np.ascontiguousarray(seq_off, np.int64)), seq_len=t(np.ascontiguousarray(seq_len, np.int32)), event_off=t(np.ascontiguousarray(event_off, np.int64)),
             mean=t(np.concatenate([np.ascontiguousarray(event_mean, np.float32), np.zeros(4, np.float32)])), model=t(np.ascontiguousarray(model).view(np.uint8)),
             scale=t(calib["scale"]), shift=t(calib["shift"]), var=t(calib["var"]), log_var=t(calib["log_var"]), trans=t(EA.trans_host(calib["events_per_base"])),
             map=t(np.ascontiguousarray(calib["map"], np.int32)), flags=t(np.ascontiguousarray(calib["flags"], np.int32)),
             cigar_off=t(np.ascontiguousarray(cg["cigar_off"], np.int64)), cigar=t(np.concatenate([cig, np.zeros(4, np.uint32)]).view(np.int32)),
             pos=t(np.ascontiguousarray(cg["pos"], np.int32)), rc=t(np.ascontiguousarray(cg["rc"], np.uint8)), ref_off=t(np.ascontiguousarray(cg["ref_off"], np.int64)),
             ref_len=t(np.ascontiguousarray(cg["ref_len"], np.int32)), ref=t(np.concatenate([np.ascontiguousarray(cg["ref_arena"], np.uint8), np.zeros(16, np.uint8)])))
    near, rec_off = torch.zeros_like(d["map"]), torch.zeros(n + 1, dtype=torch.int64, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    N.check(AC._lib().gbx_abea_event_record_device(AC.PASS_COUNT, n, d["cigar_off"].data_ptr(), d["cigar"].data_ptr(), d["pos"].data_ptr(), d["rc"].data_ptr(),
                                                   d["seq_off"].data_ptr(), d["seq_len"].data_ptr(), d["map"].data_ptr(), d["flags"].data_ptr(), near.data_ptr(),
                                                   rec_off.data_ptr(), None, 0, s))
    n_ev = np.diff(event_off)
    ordr = t(np.argsort(-n_ev, kind="stable").astype(np.int32)) if order else None
    rec = torch.full((max(total, 1) + 8, 3), -77, dtype=torch.int32, device=dev)
    n_rec, status = torch.full((n,), -7, dtype=torch.int32, device=dev), torch.full((n,), -7, dtype=torch.int32, device=dev)
    counts = torch.full((n, 3), -7, dtype=torch.int64, device=dev)
    wb = int(EA._lib().gbx_abea_eventalign_workspace_bytes(n, n_cig, rows_cap))
    work = torch.zeros(wb, dtype=torch.uint8, device=dev)
    N.check(EA._lib().gbx_abea_eventalign_device(
        n, d["seq_off"].data_ptr(), d["seq_len"].data_ptr(), d["event_off"].data_ptr(), d["mean"].data_ptr(), d["model"].data_ptr(), d["scale"].data_ptr(),
        d["shift"].data_ptr(), d["var"].data_ptr(), d["log_var"].data_ptr(), d["trans"].data_ptr(), d["map"].data_ptr(), near.data_ptr(), d["flags"].data_ptr(),
        d["cigar_off"].data_ptr(), d["cigar"].data_ptr(), d["pos"].data_ptr(), d["rc"].data_ptr(), d["ref_off"].data_ptr(), d["ref_len"].data_ptr(),
        d["ref"].data_ptr(), int(region[0]), int(region[1]), ordr.data_ptr() if order else None, rec.data_ptr(), n_rec.data_ptr(), status.data_ptr(),
        counts.data_ptr(), n_cig, rows_cap, work.data_ptr(), wb, s))
    torch.cuda.synchronize()
    out = rec.cpu().numpy()
    assert (out[total:] == -77).all()                      # nothing is written behind the reads' room
    return dict(rec=out[:total].copy().view(EA.REC_DTYPE).reshape(-1), n_rec=n_rec.cpu().numpy(), status=status.cpu().numpy(), counts=counts.cpu().numpy())


def _assert_equal(got, want, event_off, counts=True):
    assert np.array_equal(got["n_rec"], want["n_rec"]) and np.array_equal(got["status"], want["status"])
    for r in range(len(want["n_rec"])):
        assert np.array_equal(R.read_records(got, event_off, r), R.read_records(want, event_off, r)), r
    if counts:
        assert np.array_equal(got["counts"], want["counts"])


@pytest.fixture(scope="module")
def edge():
    b = R.edge_batch()
    args = (b["seq_off"], b["seq_len"], b["event_off"], b["events"]["mean"], b["model"], b["calib"], b["cg"])
    return b, args, R.run(*args, rows_cap=R.EDGE_ROWS_CAP), R.run(*args)


def test_golden_reads_device_and_host():
    g, calib, cg = golden()
    for region, idx in golden_groups(g):
        so, sl, eoff, ev, c, s = subset(g, calib, cg, idx)
        want = R.run(so, sl, eoff, ev["mean"], g["model"], c, s, region)
        dev = _device_eventalign(so, sl, eoff, ev["mean"], g["model"], c, s, region)
        host = EA.eventalign_host(so, sl, eoff, ev, g["model"], c, s, region)
        for got in (dev, host):
            assert_records_equal_golden(g, idx, got, eoff)
            _assert_equal(got, want, eoff, counts=got is dev)


def test_golden_summary_and_tsv_of_the_device_records():
    g, calib, cg = golden()
    region, idx = golden_groups(g)[0]
    assert region == (-1, -1)
    so, sl, eoff, ev, c, s = subset(g, calib, cg, idx)
    o = EA.eventalign_host(so, sl, eoff, ev, g["model"], c, s, region)
    got = EA.summary(eoff, ev, g["model"], c["scale"], c["shift"], c["var"], s, o)
    for f in got.dtype.names:
        a, b = got[f], g["summary"][f][idx]
        assert np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b), f
    tsv = g["tsv"].tobytes()
    for j, r in enumerate(idx):
        ref = s["ref_arena"][s["ref_off"][j]:s["ref_off"][j] + s["ref_len"][j]]
        for v in range(4):
            want = tsv[g["tsv_off"][4 * r + v]:g["tsv_off"][4 * r + v + 1]]
            text = EA.tsv(ev[eoff[j]:eoff[j + 1]], g["model"], c["scale"][j], c["shift"][j], c["var"][j], s["rc"][j], s["pos"][j], ref, R.read_records(o, eoff, j),
                          header=r == 0, print_read_names=bool(v & 1), scale_events=bool(v & 2), read_index=7 + r, read_name=b"read", ref_name=b"chr1")
            assert text == want, (str(g["names"][r]), v)
    with pytest.raises(N.GbxError):                         # the reference asserts
        EA.tsv(ev[:eoff[1]], g["model"], 1.0, 0.0, 1.0, 0, s["pos"][0], b"ACGTACGT", R.read_records(o, eoff, 0)[:0], write_samples=True)


def test_edge_batch_device_equals_restatement(edge):
    b, args, want_cap, _ = edge
    at = {nm: i for i, nm in enumerate(b["names"])}
    over = [at["rows %d, rc %d" % (R.EDGE_ROWS_CAP + 1, rc)] for rc in (0, 1)]
    got = _device_eventalign(*args, rows_cap=R.EDGE_ROWS_CAP)
    assert (got["status"][over] == EA.ST_ROWS).all() and (np.delete(got["status"], over) == 0).all()       # the cap + 1 reads carry the bit and nothing else does
    for rc in (0, 1):
        assert got["n_rec"][at["rows %d, rc %d" % (R.EDGE_ROWS_CAP, rc)]] == R.EDGE_ROWS_CAP - 1 and got["n_rec"][at["rows 3, rc %d" % rc]] == 2
        assert got["counts"][at["12 bases, 12 rows, rc %d" % rc]].tolist()[:2] == [1, 3 * 12 * 7]          # 7 k-mers
        assert got["counts"][at["101 bases then 40, rc %d" % rc]][0] == 2                                 # 96 k-mers, then the rest
    assert got["n_rec"][at["flagged"]] == 0 and got["n_rec"][at["no events"]] == 0
    _assert_equal(got, want_cap, b["event_off"])
    _assert_equal(_device_eventalign(*args, rows_cap=R.EDGE_ROWS_CAP, order=False), want_cap, b["event_off"])


def test_edge_batch_host_entry(edge):
    b, args, _, want = edge
    assert (want["status"] == 0).all()                      # GBX_ABEA_EVENTALIGN_ROWS holds every segment of the batch
    got = EA.eventalign_host(b["seq_off"], b["seq_len"], b["event_off"], b["events"], b["model"], b["calib"], b["cg"])
    _assert_equal(got, want, b["event_off"], counts=False)


def test_batches_of_none_and_of_one(edge):
    b, args, _, want = edge
    L = EA._lib()
    assert L.gbx_abea_eventalign_device(0, *([None] * 20), -1, -1, *([None] * 5), 0, 8, None, 0, None) == 0
    none = EA.eventalign_host([], [], [0], [], b["model"], dict(b["calib"], flags=None), b["cg"])
    assert len(none["n_rec"]) == 0 and len(none["rec"]) == 0
    k = b["names"].index("several segments, rc 1")
    cg, cal = b["cg"], b["calib"]
    one_cg = dict(cigar_off=cg["cigar_off"][k:k + 2] - cg["cigar_off"][k], cigar=cg["cigar"][cg["cigar_off"][k]:cg["cigar_off"][k + 1]], pos=cg["pos"][k:k + 1],
                  rc=cg["rc"][k:k + 1], ref_off=cg["ref_off"][k:k + 1], ref_len=cg["ref_len"][k:k + 1], ref_arena=cg["ref_arena"])
    one_cal = {f: (v if f == "map" else v[k:k + 1]) for f, v in cal.items()}
    eoff = b["event_off"][k:k + 2] - b["event_off"][k]
    ev = b["events"][b["event_off"][k]:b["event_off"][k + 1]]
    for got in (_device_eventalign(b["seq_off"][k:k + 1], b["seq_len"][k:k + 1], eoff, ev["mean"], b["model"], one_cal, one_cg),
                EA.eventalign_host(b["seq_off"][k:k + 1], b["seq_len"][k:k + 1], eoff, ev, b["model"], one_cal, one_cg)):
        assert got["status"][0] == 0 and got["n_rec"][0] == want["n_rec"][k] > 500
        assert np.array_equal(R.read_records(got, eoff, 0), R.read_records(want, b["event_off"], k))


def test_spliced_cigar_is_refused(edge):
    b = edge[0]
    cg = dict(b["cg"])
    cg["cigar"] = cg["cigar"].copy()
    cg["cigar"][int(cg["cigar_off"][5]) + 1] = (9 << 4) | 3    # operation N in read 5
    with pytest.raises(N.GbxError) as e:
        EA.eventalign_host(b["seq_off"], b["seq_len"], b["event_off"], b["events"], b["model"], b["calib"], cg)
    assert e.value.code == N.GBX_ERR_ARG and "read 5" in str(e.value)


@pytest.fixture(scope="module")
def drawn():
    ss = gen_abea_raw(8, SEED, FIRST)
    cg = gen_abea_cigars(ss, SEED, FIRST)
    return ss, cg, R.eventalign_from_signal(ss, cg, threads=16)


def test_one_call_equals_the_restatements(drawn):
    ss, cg, want = drawn
    assert (want["status"] == 0).all() and (want["flags"] == 0).sum() >= 6 and (want["n_rec"] > 4000).sum() >= 6       # the draw, checked on the CPU
    got = EA.eventalign_from_signal_host(ss, cg)
    assert (got["ea_status"] == 0).all()
    assert np.array_equal(got["flags"], want["flags"]) and np.array_equal(got["status"] & 1, want["ev_status"]) and np.array_equal(got["event_off"], want["event_off"])
    for k in ("scale", "shift", "var", "log_var"):
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k
    assert np.array_equal(got["events_per_base"].view(np.uint64), want["events_per_base"].view(np.uint64))
    assert np.array_equal(got["events"], want["events"])
    _assert_equal(dict(got, status=got["ea_status"]), want, want["event_off"], counts=False)
    with pytest.raises(N.GbxError) as e:                   # an event table that is too small: the need comes back
        EA.eventalign_from_signal_host(ss, cg, event_cap=int(want["event_off"][-1]) - 1)
    assert e.value.code == N.GBX_ERR_ARG and str(int(want["event_off"][-1])) in str(e.value)


def test_device_resident_chain(drawn):
    """raw signal -> events -> scalings -> align -> calibration -> near table -> eventalign on the device: no host copy of the
    events, the pairs or the map; what crosses is the per-read calibration (for the two host logarithms) and the transitions."""
    import torch
    from genomicsbench_amd import abea_signal as AS
    ss, cg, want = drawn
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    d = AS.DeviceAbeaSignalSet(ss, dev)
    d.run(stream)
    drs, keep = d.align_set()
    drs.run(stream)
    cal = AC.DeviceAbeaCalib(d, drs, keep, cg["cigar_off"], cg["cigar"], cg["pos"], cg["rc"])
    cal.run(stream)
    cal.record_count(stream)
    ea = EA.DeviceAbeaEventalign(cal, cg["ref_off"], cg["ref_len"], cg["ref_arena"], counts=True)
    ea.run(stream)
    torch.cuda.synchronize()
    got = ea.results()
    _assert_equal(got, want, want["event_off"], counts=False)
    assert np.array_equal(ea.counts.cpu().numpy(), want["counts"])
