"""abea host entries: the argument checks the seven host entries share, pinned by return code and full error text.  Every check
runs before the device is asked for, so none of this needs a GPU.

The batch: two reads of seven and eight bases, 10 and 12 events, CIGARs 7M and 8M, reference segments of seven and eight bases.
Each case spoils one array of it and goes to every entry that checks that array."""
import numpy as np
import pytest

from genomicsbench_amd import _native as N
from genomicsbench_amd import abea_calib as AC
from genomicsbench_amd import abea_eventalign as AE
from genomicsbench_amd.abea import EVENT_DTYPE, MODEL_DTYPE, PAIR_DTYPE
from genomicsbench_amd.abea_meth import NMODEL_CPG, SITE_DTYPE

ARG, UNSUPPORTED = N.GBX_ERR_ARG, N.GBX_ERR_UNSUPPORTED
M, SPLICE = 0, 3                                             # CIGAR operations


def _batch(**spoil):
    i64, i32, f32 = np.int64, np.int32, np.float32
    b = dict(
        n=2, seq_off=np.array([0, 8], i64), seq_len=np.array([7, 8], i32), seq_arena=np.frombuffer(b"ACGTACGAGTCATGCA", np.uint8).copy(),
        seq_bytes=16, event_off=np.array([0, 10, 22], i64), events=np.zeros(22, EVENT_DTYPE), models=np.zeros(4096, MODEL_DTYPE),
        cpg_model=np.zeros(NMODEL_CPG, MODEL_DTYPE), pairs=np.zeros(44, PAIR_DTYPE), n_pairs=np.zeros(2, i32),
        scale=np.ones(2, f32), shift=np.zeros(2, f32), var=np.ones(2, f32), log_var=np.zeros(2, f32), events_per_base=np.full(2, 1.5),
        map=np.full((16, 2), -1, i32), flags=np.zeros(2, i32),
        cigar_off=np.array([0, 1, 2], i64), cigar=np.array([7 << 4 | M, 8 << 4 | M], np.uint32), pos=np.array([100, 200], i32),
        rc=np.array([0, 1], np.uint8), ref_off=np.array([0, 7], i64), ref_len=np.array([7, 8], i32),
        ref_arena=np.frombuffer(b"ACGTACGACGTACGA", np.uint8).copy(), region=(-1, -1),
        raw=np.zeros(110, np.int16), raw_off=np.array([0, 50, 110], i64), range=np.full(2, 1400.0, f32), digitisation=np.full(2, 8192.0, f32),
        offset=np.zeros(2, f32))
    b.update(spoil)
    return b


def _out():
    """room for every output of every entry"""
    i64, i32, f32 = np.int64, np.int32, np.float32
    return dict(pairs=np.zeros(256, PAIR_DTYPE), n_pairs=np.zeros(2, i32), event_off=np.zeros(3, i64), events=np.zeros(128, EVENT_DTYPE),
                total=np.zeros(1, i64), scale=np.zeros(2, f32), shift=np.zeros(2, f32), var=np.zeros(2, f32), log_var=np.zeros(2, f32),
                var64=np.zeros(2), map=np.zeros((16, 2), i32), events_per_base=np.zeros(2), n_ea=np.zeros(2, i32), n_m=np.zeros(2, i32),
                flags=np.zeros(2, i32), status=np.zeros(2, i32), rec_off=np.zeros(3, i64), rec=np.zeros(128, PAIR_DTYPE),
                ea_rec=np.zeros(128, AE.REC_DTYPE), n_rec=np.zeros(2, i32), ea_status=np.zeros(2, i32), sites=np.zeros(64, SITE_DTYPE),
                scores=np.zeros(128, f32))


def _align(b, o):
    p = N.ptr
    return N.lib().gbx_abea_align_host(b["n"], p(b["seq_off"]), p(b["seq_len"]), p(b["seq_arena"]), b["seq_bytes"], p(b["event_off"]), p(b["events"]),
                                       p(b["models"]), p(b["scale"]), p(b["shift"]), p(o["pairs"]), p(o["n_pairs"]))


def _signal_align(b, o):
    p = N.ptr
    return N.lib().gbx_abea_signal_align_host(b["n"], p(b["raw"]), p(b["raw_off"]), p(b["range"]), p(b["digitisation"]), p(b["offset"]), p(b["seq_off"]),
                                              p(b["seq_len"]), p(b["seq_arena"]), b["seq_bytes"], p(b["models"]), p(o["event_off"]), p(o["events"]), 128,
                                              p(o["total"]), p(o["scale"]), p(o["shift"]), p(o["status"]), p(o["pairs"]), p(o["n_pairs"]))


def _calib(b, o):
    p = N.ptr
    o["scale"][:], o["shift"][:] = b["scale"], b["shift"]
    return AC._lib().gbx_abea_calib_host(b["n"], p(b["seq_off"]), p(b["seq_len"]), p(b["seq_arena"]), b["seq_bytes"], p(b["event_off"]), p(b["events"]),
                                         p(b["models"]), p(b["pairs"]), p(b["n_pairs"]), p(o["scale"]), p(o["shift"]), p(o["var"]), p(o["log_var"]),
                                         p(o["var64"]), p(o["map"]), p(o["events_per_base"]), p(o["n_ea"]), p(o["n_m"]), p(o["flags"]))


def _record(b, o):
    p = N.ptr
    return AC._lib().gbx_abea_event_record_host(b["n"], p(b["cigar_off"]), p(b["cigar"]), p(b["pos"]), p(b["rc"]), p(b["seq_off"]), p(b["seq_len"]),
                                                b["seq_bytes"], p(b["map"]), p(b["flags"]), p(o["rec_off"]), 128, p(o["rec"]), p(o["total"]))


def _eventalign(b, o):
    p = N.ptr
    return N.lib().gbx_abea_eventalign_host(b["n"], p(b["seq_off"]), p(b["seq_len"]), b["seq_bytes"], p(b["event_off"]), p(b["events"]), p(b["models"]),
                                            p(b["scale"]), p(b["shift"]), p(b["var"]), p(b["log_var"]), p(b["events_per_base"]), p(b["map"]), p(b["flags"]),
                                            p(b["cigar_off"]), p(b["cigar"]), p(b["pos"]), p(b["rc"]), p(b["ref_off"]), p(b["ref_len"]), p(b["ref_arena"]),
                                            b["region"][0], b["region"][1], p(o["ea_rec"]), p(o["n_rec"]), p(o["ea_status"]))


def _from_signal(b, o):
    p = N.ptr
    return N.lib().gbx_abea_eventalign_from_signal_host(
        b["n"], p(b["raw"]), p(b["raw_off"]), p(b["range"]), p(b["digitisation"]), p(b["offset"]), p(b["seq_off"]), p(b["seq_len"]), p(b["seq_arena"]),
        b["seq_bytes"], p(b["models"]), p(b["cigar_off"]), p(b["cigar"]), p(b["pos"]), p(b["rc"]), p(b["ref_off"]), p(b["ref_len"]), p(b["ref_arena"]),
        b["region"][0], b["region"][1], p(o["flags"]), p(o["status"]), p(o["scale"]), p(o["shift"]), p(o["var"]), p(o["log_var"]),
        p(o["events_per_base"]), p(o["event_off"]), p(o["events"]), 128, p(o["total"]), p(o["ea_rec"]), p(o["n_rec"]), p(o["ea_status"]))


def _call_meth(b, o):
    p = N.ptr
    return AC._lib().gbx_abea_call_methylation_host(
        b["n"], p(b["raw"]), p(b["raw_off"]), p(b["range"]), p(b["digitisation"]), p(b["offset"]), p(b["seq_off"]), p(b["seq_len"]), p(b["seq_arena"]),
        b["seq_bytes"], p(b["models"]), p(b["cpg_model"]), p(b["cigar_off"]), p(b["cigar"]), p(b["pos"]), p(b["rc"]), p(b["ref_off"]), p(b["ref_len"]),
        p(b["ref_arena"]), p(o["flags"]), p(o["status"]), p(o["scale"]), p(o["shift"]), p(o["var"]), p(o["events_per_base"]), 64, p(o["sites"]),
        p(o["scores"]), p(o["total"]))


ENTRY = {"gbx_abea_align_host": _align, "gbx_abea_signal_align_host": _signal_align, "gbx_abea_calib_host": _calib,
         "gbx_abea_event_record_host": _record, "gbx_abea_eventalign_host": _eventalign,
         "gbx_abea_eventalign_from_signal_host": _from_signal, "gbx_abea_call_methylation_host": _call_meth}
ALL = tuple(ENTRY)
WITH_EVENTS = ("gbx_abea_align_host", "gbx_abea_calib_host", "gbx_abea_eventalign_host")
WITH_CIGARS = ("gbx_abea_event_record_host", "gbx_abea_eventalign_host", "gbx_abea_eventalign_from_signal_host", "gbx_abea_call_methylation_host")
WITH_REFS = WITH_CIGARS[1:]
WITH_REGION = WITH_REFS[:2]


def _fails(entry, spoil, code, text):
    rc = ENTRY[entry](_batch(**spoil), _out())
    assert rc == code, (entry, rc)
    assert N.lib().gbx_last_error().decode() == text.replace("WHO", entry)


@pytest.mark.parametrize("entry", ALL)
@pytest.mark.parametrize("spoil", [dict(seq_off=np.array([0, 9], np.int64)), dict(seq_off=np.array([0, -1], np.int64)), dict(seq_bytes=15)],
                         ids=["past_the_end", "below_zero", "short_arena"])
def test_read_outside_the_arena(entry, spoil):
    _fails(entry, spoil, ARG, "WHO: read 1 lies outside the arena")


@pytest.mark.parametrize("entry", WITH_EVENTS)
def test_event_off_not_monotone(entry):
    _fails(entry, dict(event_off=np.array([0, 10, 5], np.int64)), ARG, "WHO: event_off not monotone at read 1")


@pytest.mark.parametrize("entry", WITH_EVENTS)
def test_event_off_below_zero(entry):
    """align's own check names read 0; the later entries look at event_off[0] first"""
    text = "WHO: event_off not monotone at read 0" if entry == "gbx_abea_align_host" else "WHO: event_off below 0"
    _fails(entry, dict(event_off=np.array([-1, 10, 22], np.int64)), ARG, text)


@pytest.mark.parametrize("entry", WITH_EVENTS[1:])
def test_too_many_events(entry):
    _fails(entry, dict(event_off=np.array([0, 10, 11 + (1 << 30)], np.int64)), UNSUPPORTED, "WHO: read 1 has too many events")


@pytest.mark.parametrize("entry", ALL)
def test_read_shorter_than_a_kmer(entry):
    spoil = dict(seq_len=np.array([7, 5], np.int32), cigar=np.array([7 << 4 | M, 5 << 4 | M], np.uint32))
    if entry == "gbx_abea_align_host":                      # its plan speaks, and asks for an event as well
        _fails(entry, spoil, ARG, "gbx_abea_plan_host: read 1 needs at least one event and 6 bases")
    else:
        _fails(entry, spoil, ARG, "WHO: read 1 needs at least 6 bases")


SPLICED = dict(cigar_off=np.array([0, 1, 4], np.int64), cigar=np.array([7 << 4 | M, 4 << 4 | M, 10 << 4 | SPLICE, 4 << 4 | M], np.uint32))
BAD_REF = dict(ref_len=np.array([7, -1], np.int32))


@pytest.mark.parametrize("entry", WITH_CIGARS)
def test_spliced_cigar(entry):
    _fails(entry, SPLICED, ARG, "WHO: read 1: a spliced alignment (operation N)")


@pytest.mark.parametrize("entry", WITH_REFS)
@pytest.mark.parametrize("spoil", [BAD_REF, dict(ref_off=np.array([0, -7], np.int64))], ids=["length", "offset"])
def test_negative_reference_segment(entry, spoil):
    _fails(entry, spoil, ARG, "WHO: bad reference segment at read 1")


@pytest.mark.parametrize("entry", WITH_REGION)
def test_region_start_above_end(entry):
    _fails(entry, dict(region=(5, 4)), ARG, "WHO: region 5 .. 4")


def test_order_of_the_checks():
    """two spoiled arrays in one call: which check speaks"""
    both = dict(SPLICED, **BAD_REF)
    _fails("gbx_abea_call_methylation_host", both, ARG, "WHO: bad reference segment at read 1")        # the segments before the CIGARs
    _fails("gbx_abea_eventalign_host", both, ARG, "WHO: read 1: a spliced alignment (operation N)")      # the CIGARs before the segments
    _fails("gbx_abea_eventalign_from_signal_host", both, ARG, "WHO: read 1: a spliced alignment (operation N)")
    _fails("gbx_abea_eventalign_host", dict(BAD_REF, region=(5, 4)), ARG, "WHO: region 5 .. 4")           # the region before the segments
    # read by read: a bad read 0 speaks before a worse read 1, whatever the check
    early = dict(event_off=np.array([0, -3, 22], np.int64), seq_off=np.array([0, 9], np.int64))
    for entry in WITH_EVENTS:
        _fails(entry, early, ARG, "WHO: event_off not monotone at read 0")
    # within a read: the arena, then the length, then the events
    late = dict(seq_off=np.array([0, 12], np.int64), seq_len=np.array([7, 5], np.int32), event_off=np.array([0, 10, 5], np.int64))
    for entry in ("gbx_abea_calib_host", "gbx_abea_signal_align_host"):
        _fails(entry, late, ARG, "WHO: read 1 lies outside the arena")
    _fails("gbx_abea_calib_host", dict(late, seq_off=np.array([0, 8], np.int64)), ARG, "WHO: read 1 needs at least 6 bases")
    # the arena before the CIGARs in the record and eventalign, the CIGARs before the arena in the two one-call entries
    mixed = dict(SPLICED, seq_off=np.array([0, 9], np.int64))
    for entry in ("gbx_abea_event_record_host", "gbx_abea_eventalign_host"):
        _fails(entry, mixed, ARG, "WHO: read 1 lies outside the arena")
    for entry in ("gbx_abea_eventalign_from_signal_host", "gbx_abea_call_methylation_host"):
        _fails(entry, mixed, ARG, "WHO: read 1: a spliced alignment (operation N)")


def test_the_batch_itself_passes_the_checks():
    """unspoiled, every entry gets as far as asking for the device"""
    if N.device_count() > 0:
        return                                              # with a device the GPU tests run these entries
    for entry in ALL:
        assert ENTRY[entry](_batch(), _out()) == N.GBX_ERR_NO_DEVICE, entry
