"""CPU restatement of abea's eventalign stage (tests/abea_eventalign_ref.c) behind numpy arrays.  Test infrastructure.

The C file states the contract of include/gbx.h (what eventalign.c:171-240, 293-338, 345-911, 919-957, 1112-1179, 1263-1540,
1580-1642 and 1853-1938 compute) with the aligned pairs and both matrices materialised, and is pinned by
tests/golden/abea_eventalign.npz; it is built here on first use, next to this file or, where that is not writable, in a
temporary directory.  ``eventalign_from_signal`` composes the restatements of all the abea stages into what
gbx_abea_eventalign_from_signal_host computes.  ``make_batch`` builds hand-made reads: the edge batch of the GPU tests and the
inputs the golden file was recorded from.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from genomicsbench_amd.abea import EVENT_DTYPE, MODEL_DTYPE, PAIR_DTYPE, KMER
from genomicsbench_amd.abea_eventalign import REC_DTYPE, SUMMARY_DTYPE

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None
ROWS_CAP = 1024


def _L():
    global _lib
    if _lib is None:
        src = os.path.join(_HERE, "abea_eventalign_ref.c")
        out = os.path.join(_HERE, "libabea_eventalign_ref.so")
        if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
            if not os.access(_HERE, os.W_OK):
                out = os.path.join(tempfile.mkdtemp(prefix="abea_eventalign_ref"), "libabea_eventalign_ref.so")
            subprocess.run(["cc", "-O2", "-std=c11", "-ffp-contract=off", "-fopenmp", "-fPIC", "-shared", src, "-o", out, "-lm"], check=True)
        _lib = C.CDLL(out)
        vp, i64, i32, f32 = C.c_void_p, C.c_int64, C.c_int32, C.c_float
        _lib.aer_transitions.argtypes = [C.c_double, vp]
        _lib.aer_transitions.restype = None
        _lib.aer_pick.argtypes = [vp, vp]
        _lib.aer_pick.restype = i32
        _lib.aer_many.argtypes = [i64] + [vp] * 19 + [i32, i32, i32, vp, vp, vp, vp, C.c_int]
        _lib.aer_many.restype = None
        _lib.aer_summary.argtypes = [vp, vp, f32, f32, f32, C.c_int, i32, vp, vp, i32, vp]
        _lib.aer_summary.restype = None
        _lib.aer_tsv.argtypes = [vp, vp, f32, f32, f32, C.c_int, i32, vp, vp, i32, C.c_int, C.c_int, C.c_int, i64, C.c_char_p, C.c_char_p, f32, vp, i64]
        _lib.aer_tsv.restype = i64
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def transitions(events_per_base):
    t = np.zeros(10, np.float32)
    _L().aer_transitions(float(events_per_base), _p(t))
    return t


def pick(x):
    """update_cell on six candidates -> (from, max)"""
    x, mx = np.ascontiguousarray(x, np.float32), np.zeros(1, np.float32)
    assert x.size == 6
    return int(_L().aer_pick(_p(x), _p(mx))), mx[0]


def run(seq_off, seq_len, event_off, event_mean, model, calib, cg, region=(-1, -1), rows_cap=ROWS_CAP, threads=4):
    """align_read_to_ref over reads -> dict(rec REC_DTYPE[n_events]: read r's at event_off[r], n_rec, status, counts int64[n, 3]:
    segments, cells, traceback steps).  calib: dict(scale, shift, var, log_var, events_per_base, map, flags)."""
    n = len(seq_len)
    seq_off, seq_len = np.ascontiguousarray(seq_off, np.int64), np.ascontiguousarray(seq_len, np.int32)
    event_off = np.ascontiguousarray(event_off, np.int64)
    means = np.concatenate([np.ascontiguousarray(event_mean, np.float32), np.zeros(4, np.float32)])
    model = np.ascontiguousarray(model, MODEL_DTYPE)
    f = lambda k: np.ascontiguousarray(calib[k], np.float32)
    scale, shift, var, log_var = f("scale"), f("shift"), f("var"), f("log_var")
    epb, map_ = np.ascontiguousarray(calib["events_per_base"], np.float64), np.ascontiguousarray(calib["map"], np.int32)
    flags = None if calib.get("flags") is None else np.ascontiguousarray(calib["flags"], np.int32)
    cigar = np.ascontiguousarray(cg["cigar"], np.uint32) if len(cg["cigar"]) else np.zeros(1, np.uint32)
    cigar_off, pos, rc = np.ascontiguousarray(cg["cigar_off"], np.int64), np.ascontiguousarray(cg["pos"], np.int32), np.ascontiguousarray(cg["rc"], np.uint8)
    ref_off, ref_len = np.ascontiguousarray(cg["ref_off"], np.int64), np.ascontiguousarray(cg["ref_len"], np.int32)
    ref = np.concatenate([np.ascontiguousarray(cg["ref_arena"], np.uint8), np.zeros(8, np.uint8)])
    if ((cigar & 0xf) == 3).any() or ((cigar & 0xf) == 6).any() or ((cigar & 0xf) > 8).any():
        raise ValueError("the reference refuses a CIGAR operation")
    total = int(event_off[n]) if n else 0
    rec, n_rec, status, counts = np.zeros(max(total, 1), REC_DTYPE), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32), np.zeros((max(n, 1), 3), np.int64)
    _L().aer_many(n, _p(cigar_off), _p(cigar), _p(pos), _p(rc), _p(seq_off), _p(seq_len), _p(map_), _p(event_off), _p(means), _p(model), _p(scale),
                  _p(shift), _p(var), _p(log_var), _p(epb), _p(flags), _p(ref_off), _p(ref_len), _p(ref), int(region[0]), int(region[1]), int(rows_cap),
                  _p(rec), _p(n_rec), _p(status), _p(counts), threads)
    return dict(rec=rec[:total], n_rec=n_rec[:n], status=status[:n], counts=counts[:n])


def read_records(o, event_off, r):
    a = int(event_off[r] - event_off[0])
    return o["rec"][a:a + int(o["n_rec"][r])]


def _ref_of(cg, r):
    return np.ascontiguousarray(np.concatenate([np.asarray(cg["ref_arena"], np.uint8)[int(cg["ref_off"][r]):int(cg["ref_off"][r]) + int(cg["ref_len"][r])],
                                                np.zeros(8, np.uint8)]))


def summary(event_off, events, model, scale, shift, var, cg, o):
    n = len(event_off) - 1
    events, model = np.ascontiguousarray(events, EVENT_DTYPE), np.ascontiguousarray(model, MODEL_DTYPE)
    out = np.zeros(max(n, 1), SUMMARY_DTYPE)
    for r in range(n):
        q = np.ascontiguousarray(read_records(o, event_off, r))
        ev = events[int(event_off[r]):int(event_off[r + 1])]
        if len(q):
            _L().aer_summary(_p(ev), _p(model), float(scale[r]), float(shift[r]), float(var[r]), int(cg["rc"][r]), int(cg["pos"][r]), _p(_ref_of(cg, r)),
                             _p(q), len(q), _p(out[r:]))
    return out[:n]


def tsv(events, model, scale, shift, var, rc, pos, ref, rec, header=False, print_read_names=False, scale_events=False, read_index=0, read_name=b"",
        ref_name=b"contig", sample_rate=4000.0):
    events, model = np.ascontiguousarray(events, EVENT_DTYPE), np.ascontiguousarray(model, MODEL_DTYPE)
    if not len(events):
        events = np.zeros(1, EVENT_DTYPE)
    ref = np.concatenate([np.frombuffer(bytes(ref), np.uint8) if isinstance(ref, (bytes, bytearray)) else np.ascontiguousarray(ref, np.uint8), np.zeros(8, np.uint8)])
    rec = np.ascontiguousarray(rec, REC_DTYPE)
    cap = 400 + (160 + len(ref_name) + len(read_name)) * len(rec)
    text = np.zeros(cap, np.uint8)
    q = rec if len(rec) else np.zeros(1, REC_DTYPE)
    k = _L().aer_tsv(_p(events), _p(model), float(scale), float(shift), float(var), int(rc), int(pos), _p(ref), _p(q), len(rec), int(header),
                     int(print_read_names), int(scale_events), int(read_index), bytes(read_name), bytes(ref_name), float(sample_rate), _p(text), cap)
    assert k >= 0
    return text[:k].tobytes()


def eventalign_from_signal(ss, cg, region=(-1, -1), threads=16):
    """What gbx_abea_eventalign_from_signal_host computes, by the CPU restatements of every stage: abea_events_ref (events,
    scalings), the abea oracle (align), abea_calib_ref (calibration) and this file."""
    import abea_calib_ref as CR
    import abea_events_ref as ER
    from oracle import oracle_py as O
    ev = ER.run(ss, threads)
    off, means = ev["event_off"], np.ascontiguousarray(ev["events"]["mean"])
    rs, keep = ss.read_set(off, means, ev["scale"], ev["shift"])
    out, npk = O.abea_oracle(rs, threads)
    n = ss.n_reads
    pairs, n_pairs = np.zeros(2 * max(int(off[-1]), 1), PAIR_DTYPE), np.zeros(n, np.int32)
    for k, r in enumerate(keep):
        a = 2 * int(rs.event_off[k])
        pairs[2 * int(off[r]):2 * int(off[r]) + int(npk[k])] = out[a:a + int(npk[k])]
        n_pairs[r] = npk[k]
    c = CR.calibrate(ss.seq_off, ss.seq_len, ss.seq_arena, off, means, ss.model, pairs, n_pairs, ev["scale"], ev["shift"])
    o = run(ss.seq_off, ss.seq_len, off, means, ss.model, c, cg, region, ROWS_CAP, threads)
    o.update(flags=c["flags"][:n], ev_status=ev["status"], scale=c["scale"][:n], shift=c["shift"][:n], var=c["var"][:n], log_var=c["log_var"][:n],
             events_per_base=c["events_per_base"][:n], event_off=off, events=ev["events"], calib=c, event_mean=means)
    return o


# ---- hand-made reads

_ACGT = np.frombuffer(b"ACGT", np.uint8)


def _ranks(seq):
    v = np.zeros(256, np.int64); v[ord("C")], v[ord("G")], v[ord("T")] = 1, 2, 3
    c, n = v[np.asarray(seq, np.uint8)], len(seq) - KMER + 1
    return sum(c[i:i + n] * 4 ** (KMER - 1 - i) for i in range(KMER))


def _revcomp(s):
    t = np.zeros(256, np.uint8); t[:] = ord("T")
    for a, b in zip(b"ACGT", b"TGCA"):
        t[a] = b
    return t[np.asarray(s, np.uint8)][::-1].copy()


def make_batch(specs, seed, model):
    """specs: dicts(name, n (bases), ops [(len, letter)], counts (events of each of the n - 5 read k-mers, or an int for all), rc,
    and optionally flag, kick {event: pA}, epb, region (offsets from pos), lower / codes: reference positions to write in lower case / as
    IUPAC codes).  The
    CIGAR describes the read's bases (their reverse complement for rc); = and M copy them to the reference, X changes them, D
    draws bases.  Event e of read k-mer k has the mean scale x level + shift + noise.  -> dict of the entries' arrays."""
    from genomicsbench_amd.datagen import bam_cigar
    rng = np.random.default_rng(seed)
    reads = []
    for sp in specs:
        n = sp["n"]
        while True:
            seq = _ACGT[rng.integers(0, 4, n)]
            if np.all(np.diff(_ranks(seq)) != 0):
                break
        counts = np.full(n - 5, sp["counts"], np.int64) if np.isscalar(sp["counts"]) else np.asarray(sp["counts"], np.int64)
        assert len(counts) == n - 5
        rk = _ranks(seq)
        ev_k = np.repeat(np.arange(n - 5), counts)
        scale, shift = np.float32(1.0 + 0.05 * rng.random()), np.float32(4.0 * rng.random() - 2.0)
        mean = scale * model["level_mean"][rk[ev_k]] + shift + 0.3 * rng.normal(size=len(ev_k)) * model["level_stdv"][rk[ev_k]]
        for e, pa in sp.get("kick", {}).items():
            mean[e] += pa
        ev = np.zeros(len(ev_k), EVENT_DTYPE)
        ev["length"] = rng.integers(3, 40, len(ev_k)).astype(np.float32)
        ev["start"] = np.cumsum(ev["length"]).astype(np.uint64)
        ev["mean"], ev["stdv"] = mean.astype(np.float32), (0.5 + 2.0 * rng.random(len(ev_k))).astype(np.float32)
        first = np.cumsum(counts) - counts
        m = np.where((counts > 0)[:, None], np.stack([first, first + counts - 1], 1), -1).astype(np.int32)
        oriented = _revcomp(seq) if sp["rc"] else seq
        ref, rp = [], 0
        for ln, op in sp["ops"]:
            if op in "M=":
                ref.append(oriented[rp:rp + ln]); rp += ln
            elif op == "X":
                ref.append(_ACGT[(np.searchsorted(_ACGT, oriented[rp:rp + ln]) + 1 + rng.integers(0, 3, ln)) % 4]); rp += ln
            elif op == "D":
                ref.append(_ACGT[rng.integers(0, 4, ln)])
            elif op in "IS":
                rp += ln
        assert rp <= n
        ref = np.concatenate(ref + [np.zeros(0, np.uint8)]).astype(np.uint8)
        for i in sp.get("lower", []):
            ref[i] = ref[i] + 32
        for i, code in sp.get("codes", {}).items():
            ref[i] = ord(code)
        var = np.float32(1.0 + 0.2 * rng.random())
        reads.append(dict(seq=seq, ev=ev, map=m, cigar=bam_cigar(sp["ops"]), ref=ref, rc=sp["rc"], pos=1000 + 37 * len(reads), scale=scale, shift=shift,
                          var=var, log_var=np.float32(np.log(np.float64(var))), epb=sp.get("epb", max(1.2, len(ev_k) / max(n - 5, 1))),
                          flag=sp.get("flag", 0), name=sp["name"], region=sp.get("region")))
    k = len(reads)
    seq_len = np.array([len(r["seq"]) for r in reads], np.int32)
    seq_off = np.zeros(k, np.int64); seq_off[1:] = np.cumsum(seq_len[:-1] + 2)
    nb = int(seq_off[-1] + seq_len[-1]) + 8
    map_ = np.full((nb, 2), -5, np.int32)
    for o, r in zip(seq_off, reads):
        map_[o:o + len(r["map"])] = r["map"]
    off = lambda key: np.concatenate([[0], np.cumsum([len(r[key]) for r in reads])]).astype(np.int64)
    cat = lambda key, dt: np.concatenate([r[key] for r in reads] + [np.zeros(0, dt)]).astype(dt)
    col = lambda key, dt: np.array([r[key] for r in reads], dt)
    calib = dict(scale=col("scale", np.float32), shift=col("shift", np.float32), var=col("var", np.float32), log_var=col("log_var", np.float32),
                 events_per_base=col("epb", np.float64), map=map_, flags=col("flag", np.int32))
    cg = dict(cigar_off=off("cigar"), cigar=cat("cigar", np.uint32), pos=col("pos", np.int32), rc=col("rc", np.uint8), ref_off=off("ref")[:-1],
              ref_len=np.array([len(r["ref"]) for r in reads], np.int32), ref_arena=cat("ref", np.uint8))
    region = np.array([[r["pos"] + r["region"][0], r["pos"] + r["region"][1]] if r["region"] else [-1, -1] for r in reads], np.int32)
    return dict(region=region, seq_off=seq_off, seq_len=seq_len, event_off=off("ev"), events=cat("ev", EVENT_DTYPE), model=model, calib=calib, cg=cg,
                names=[r["name"] for r in reads])


def _spread(n_kmers, lo, hi, total):
    """`total` events over the k-mers lo .. hi - 1 as evenly as they go, none elsewhere"""
    c = np.zeros(n_kmers, np.int64)
    c[lo:hi] = total // (hi - lo)
    c[lo:lo + total % (hi - lo)] += 1
    return c


EDGE_ROWS_CAP = 200


def edge_specs():
    """The edge batch of the GPU tests, every shape on both strands: segments of 12 and of 101 bases (7 and 96 k-mers), rows of 3,
    63, 64, 65 and EDGE_ROWS_CAP - 1, EDGE_ROWS_CAP, EDGE_ROWS_CAP + 1, a read of several segments, a read of more than 64
    operations, a flagged read and a read without events."""
    sp = []

    def rows_read(name, rows, rc):
        # 7S 12M 12S of 31 bases: the aligned read positions 7 .. 18 flip onto themselves (7 + 18 = 31 - 6), so on either strand the
        # segment's events run between the first events of read k-mers 7 and 18: rows = 1 + the events of k-mers 7 .. 17
        c = _spread(26, 7, 18, rows - 1)
        c[18] = 1
        sp.append(dict(name="%s, rc %d" % (name, rc), n=31, ops=[(7, "S"), (12, "M"), (12, "S")], counts=c, rc=rc, epb=2.0))

    for rc in (0, 1):
        rows_read("12 bases, 12 rows", 12, rc)
        for rows in (3, 63, 64, 65, EDGE_ROWS_CAP - 1, EDGE_ROWS_CAP, EDGE_ROWS_CAP + 1):
            rows_read("rows %d" % rows, rows, rc)
        sp.append(dict(name="101 bases then 40, rc %d" % rc, n=160, ops=[(10, "S"), (141, "M"), (9, "S")], counts=1, rc=rc))
        sp.append(dict(name="several segments, rc %d" % rc, n=420, ops=[(4, "H"), (6, "S"), (150, "="), (2, "I"), (120, "M"), (3, "D"), (130, "M"), (12, "S")],
                       counts=np.tile([1, 2, 1, 1, 3, 1, 0, 2], 52)[:415], rc=rc))
        sp.append(dict(name="more than 64 operations, rc %d" % rc, n=500, ops=[(4, "M"), (1, "I"), (3, "="), (1, "D")] * 60 + [(20, "S")], counts=1, rc=rc))
    sp.append(dict(name="flagged", n=200, ops=[(200, "M")], counts=1, rc=0, flag=4))
    sp.append(dict(name="no events", n=100, ops=[(100, "M")], counts=0, rc=0))
    return sp


def edge_batch():
    from genomicsbench_amd.datagen import gen_abea
    return make_batch(edge_specs(), 60606, gen_abea(1, 5001).model)


def golden_specs():
    """What tests/golden/abea_eventalign.npz was recorded from (the reference's own eventalign.c ran on make_batch(golden_specs(),
    777, model)); kept so that the file can be understood and remade."""
    sp = []
    for rc in (0, 1):
        sp.append(dict(name="one segment, rc %d" % rc, n=96, ops=[(8, "S"), (80, "M"), (8, "S")], counts=np.tile([1, 2], 46)[:91], rc=rc))
        for emitted in (49, 50, 51):
            # the first segment ends at the pair 100 reference bases on: read k-mer 100 (forward); rows = 1 + the events before it
            c = np.ones(295, np.int64)
            lo = 194 if rc else 0                                   # rc: the first pair is read k-mer 294, the pair 100 bases on k-mer 194
            c[lo:lo + 100] = 0
            c[lo + (np.arange(emitted) * 100) // emitted] = 1
            sp.append(dict(name="%d states before the cut, rc %d" % (emitted, rc), n=300, ops=[(300, "M")], counts=c, rc=rc))
        sp.append(dict(name="outlier event, rc %d" % rc, n=150, ops=[(150, "M")], counts=3, rc=rc, kick={100: 45.0, 217: -50.0}, epb=3.0))
        sp.append(dict(name="deleted bases, rc %d" % rc, n=220, ops=[(3, "H"), (70, "M"), (1, "D"), (60, "="), (2, "D"), (90, "M")], counts=np.tile([2, 1, 1], 72)[:215], rc=rc))
        sp.append(dict(name="insertion, rc %d" % rc, n=330, ops=[(5, "S"), (90, "M"), (80, "I"), (150, "M"), (5, "S")], counts=np.tile([1, 2, 1, 1], 82)[:325], rc=rc))
        sp.append(dict(name="deletion of 130, rc %d" % rc, n=330, ops=[(160, "M"), (130, "D"), (170, "M")], counts=1, rc=rc))
        sp.append(dict(name="region trim, rc %d" % rc, n=350, ops=[(20, "S"), (330, "M")], counts=np.tile([1, 2, 1], 115)[:345], rc=rc, region=(60, 260)))
        c = np.ones(345, np.int64); c[150:290] = 0
        sp.append(dict(name="140 k-mers without events, rc %d" % rc, n=350, ops=[(350, "M")], counts=c, rc=rc))
        # one event is left behind the last segment that emits: the next segment's events are 1 apart and the read ends there (|start - stop| < 2)
        c = np.ones(295, np.int64); c[200:] = 0; c[290] = 1
        sp.append(dict(name="ends one event short, rc %d" % rc, n=300, ops=[(300, "M")], counts=c[::-1].copy() if rc else c, rc=rc))
    sp.append(dict(name="lower case and codes", n=250, ops=[(6, "H"), (10, "S"), (100, "M"), (4, "X"), (126, "M"), (10, "S")], counts=np.tile([1, 1, 2], 82)[:245], rc=0,
                   lower=list(range(20, 60)), codes={7: "N", 30: "R", 31: "y", 90: "K", 140: "S", 141: "n", 200: "B", 201: "M"}))
    return sp
