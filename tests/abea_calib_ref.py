"""CPU restatement of abea's calibration and event-alignment record (tests/abea_calib_ref.c) behind numpy arrays.  Test
infrastructure.

The C file states the contract of include/gbx.h (what align.c:550-762, f5c.c:1262-1330 and meth.c:15-185 compute) in serial
loops over flat arrays and is pinned by the two golden files; it is built here on first use, next to this file or, where that is not writable, in a temporary directory.  ``call_methylation`` composes the
restatements of all the abea stages into what gbx_abea_call_methylation_host computes.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from genomicsbench_amd.abea import PAIR_DTYPE, KMER

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


def _L():
    global _lib
    if _lib is None:
        src = os.path.join(_HERE, "abea_calib_ref.c")
        out = os.path.join(_HERE, "libabea_calib_ref.so")
        if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
            if not os.access(_HERE, os.W_OK):
                out = os.path.join(tempfile.mkdtemp(prefix="abea_calib_ref"), "libabea_calib_ref.so")
            subprocess.run(["cc", "-O2", "-std=c11", "-ffp-contract=off", "-fPIC", "-shared", src, "-o", out, "-lm"], check=True)
        _lib = C.CDLL(out)
        vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
        _lib.acr_calib_many.argtypes = [i64] + [vp] * 18
        _lib.acr_calib_many.restype = None
        _lib.acr_record_read.argtypes = [vp, i64, i32, C.c_int, i32, vp, vp]
        _lib.acr_record_read.restype = i32
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


CALIB_FIELDS = ("scale", "shift", "var", "log_var", "var64", "map", "events_per_base", "n_event_alignment", "n_m_state", "flags")


def calibrate(seq_off, seq_len, seq_arena, event_off, event_mean, model, pairs, n_pairs, scale, shift):
    """scaling_single over reads -> dict of CALIB_FIELDS; map is int32[len(seq_arena), 2], read r's entries at seq_off[r]."""
    n = len(seq_len)
    seq_off, event_off = np.ascontiguousarray(seq_off, np.int64), np.ascontiguousarray(event_off, np.int64)
    seq_len, n_pairs = np.ascontiguousarray(seq_len, np.int32), np.ascontiguousarray(n_pairs, np.int32)
    seq_arena = np.ascontiguousarray(seq_arena, np.uint8)
    means = np.concatenate([np.ascontiguousarray(event_mean, np.float32), np.zeros(4, np.float32)])
    pairs = np.ascontiguousarray(pairs, PAIR_DTYPE) if len(pairs) else np.zeros(2, PAIR_DTYPE)
    z = lambda dt: np.zeros(max(n, 1), dt)
    o = dict(scale=np.array(scale, np.float32).copy(), shift=np.array(shift, np.float32).copy(), var=z(np.float32), log_var=z(np.float32),
             var64=z(np.float64), map=np.full((len(seq_arena), 2), -7, np.int32), events_per_base=z(np.float64), n_event_alignment=z(np.int32),
             n_m_state=z(np.int32), flags=z(np.int32))
    _L().acr_calib_many(n, _p(seq_off), _p(seq_len), _p(seq_arena), _p(event_off), _p(means), _p(np.ascontiguousarray(model)), _p(pairs), _p(n_pairs),
                        *[_p(o[k]) for k in CALIB_FIELDS])
    return o


def record(cigar_off, cigar, pos, rc, seq_off, seq_len, map_, flags=None):
    """get_event_alignment_record over reads -> (rec_off int64[n + 1], rec PAIR_DTYPE[]); ValueError where the reference refuses"""
    n = len(seq_len)
    cigar = np.ascontiguousarray(cigar, np.uint32) if len(cigar) else np.zeros(1, np.uint32)
    map_ = np.ascontiguousarray(map_, np.int32)
    recs, rec_off = [], np.zeros(n + 1, np.int64)
    for r in range(n):
        rec_off[r + 1] = rec_off[r]
        if flags is not None and flags[r]:
            continue
        out = np.zeros(max(int(seq_len[r]), 1), PAIR_DTYPE)
        k = _L().acr_record_read(_p(cigar[int(cigar_off[r]):]), int(cigar_off[r + 1] - cigar_off[r]), int(pos[r]), int(rc[r]), int(seq_len[r]),
                                 _p(map_[int(seq_off[r]):]), _p(out))
        if k < 0:
            raise ValueError("read %d: the reference refuses its CIGAR" % r)
        recs.append(out[:k])
        rec_off[r + 1] += k
    return rec_off, (np.concatenate(recs) if recs else np.zeros(0, PAIR_DTYPE))


def read_maps(map_, seq_off, seq_len):
    """the entries of a map that belong to reads (the slots between them are unspecified)"""
    return np.concatenate([map_[int(o):int(o) + int(l) - KMER + 1] for o, l in zip(seq_off, seq_len)] + [np.zeros((0, 2), np.int32)])


def call_methylation(ss, cg, threads=16):
    """What gbx_abea_call_methylation_host computes, by the CPU restatements of every stage: abea_events_ref (events, scalings), the
    abea oracle (align), this file (calibration, record) and abea_meth_ref (planner, score).  ss: an AbeaSignalSet, cg: the
    dict of datagen.gen_abea_cigars.  -> dict(flags, status, scale, shift, var, events_per_base, sites, scores)."""
    import abea_events_ref as ER
    import abea_meth_ref as MR
    from genomicsbench_amd.abea_meth import AbeaMethJobSet
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
    c = calibrate(ss.seq_off, ss.seq_len, ss.seq_arena, off, means, ss.model, pairs, n_pairs, ev["scale"], ev["shift"])
    rec_off, rec = record(cg["cigar_off"], cg["cigar"], cg["pos"], cg["rc"], ss.seq_off, ss.seq_len, c["map"], c["flags"])
    sites, jobs, arena = MR.sites(cg["ref_off"], cg["ref_len"], cg["ref_arena"], cg["pos"], cg["rc"], rec_off, rec)
    js = AbeaMethJobSet(jobs, arena, off, means, c["scale"], c["shift"], c["var"], c["log_var"], c["events_per_base"], cg["cpg_model"])
    scores = MR.score(js, threads)[0] if js.n_jobs else np.zeros(0, np.float32)
    return dict(flags=c["flags"][:n], status=ev["status"], scale=c["scale"][:n], shift=c["shift"][:n], var=c["var"][:n],
                events_per_base=c["events_per_base"][:n], sites=sites, scores=scores, rec_off=rec_off, rec=rec, calib=c, event_off=off,
                event_mean=means, pairs=pairs, n_pairs=n_pairs)


def _kmer_ranks(seq):
    v = np.zeros(256, np.int64); v[ord("C")], v[ord("G")], v[ord("T")] = 1, 2, 3
    c, n = v[np.asarray(seq, np.uint8)], len(seq) - KMER + 1
    return sum(c[i:i + n] * 4 ** (KMER - 1 - i) for i in range(KMER))


def edge_calib_set():
    """The edge batch of the calibration tests: hand-made monotone pair lists (not from align()).  A read is its bases, the
    number of events of each k-mer and how a k-mer without events appears in the list (not at all, or as a pair that repeats
    the event before it); event e of k-mer k has the mean scale x level + shift + noise.  -> (AbeaReadSet, pairs in the
    2 x event_off layout, n_pairs, names)."""
    from genomicsbench_amd.abea import AbeaReadSet
    from genomicsbench_amd.datagen import gen_abea
    model = gen_abea(1, 5001).model
    rng = np.random.default_rng(90210)
    acgt = np.frombuffer(b"ACGT", np.uint8)

    def bases(n):
        while True:
            s = acgt[rng.integers(0, 4, n)]
            if n < 7 or np.all(np.diff(_kmer_ranks(s)) != 0):
                return s

    reads, names = [], []

    def add(name, seq, counts, noise=0.3, kick=0.0, repeat_style=True, dup=False, drop=False):
        seq = np.asarray(seq, np.uint8)
        counts = np.asarray(counts, np.int64)
        rk = _kmer_ranks(np.where(np.isin(seq, acgt), seq, ord("A")).astype(np.uint8))
        ev_k = np.repeat(np.arange(len(counts)), counts)
        mean = 1.03 * model["level_mean"][rk[ev_k]] - 2.0 + noise * rng.normal(size=len(ev_k)) * model["level_stdv"][rk[ev_k]]
        mean = mean + kick * np.where(rng.random(len(ev_k)) < 0.5, 1.0, -1.0)
        first = np.cumsum(counts) - counts
        pr = []
        for k, c in enumerate(counts):
            if c == 0:
                if repeat_style and pr and k % 3:                       # a skip: the k-mer repeats the event before it
                    pr.append((k, pr[-1][1]))
                continue
            if pr and k % 5 == 0 and repeat_style:                      # its first pair repeats the event before it, then its own
                pr.append((k, pr[-1][1]))
            for e in range(first[k], first[k] + c):
                pr.append((k, e))
                if dup and e % 7 == 0:
                    pr.append((k, e))                                    # the same pair twice
        if drop:
            pr = []
        reads.append((seq, mean.astype(np.float32), np.array(pr, np.int32).reshape(-1, 2)))
        names.append(name)

    add("no pairs", bases(50), np.ones(45), drop=True)
    for n in (6, 68, 69, 70):
        add("%d bases" % n, bases(n), np.ones(n - 5))
    add("199 M states", bases(204), np.ones(199), repeat_style=False)
    add("200 M states", bases(205), np.ones(200), repeat_style=False)
    add("homopolymer", np.full(300, ord("A"), np.uint8), np.ones(295))
    c = np.ones(700, np.int64); c[40:75] = 0; c[200:330] = 0; c[331:333] = 0; c[690:] = 0
    add("runs without events", bases(705), c)
    add("runs without events, pairs left out", bases(705), c, repeat_style=False)
    add("several events per k-mer", bases(405), rng.integers(1, 5, 400), dup=True)
    add("60 pA off", bases(505), np.ones(500), kick=60.0)
    add("var under 2.5", bases(3005), np.ones(3000), noise=2.40, repeat_style=False)
    add("var over 2.5", bases(3005), np.ones(3000), noise=2.60, repeat_style=False)
    add("events_per_base under 5", bases(305), np.full(300, 5), repeat_style=False)
    c = np.full(300, 5); c[[10, 200]] = 6
    add("events_per_base over 5", bases(305), c, repeat_style=False)
    s = bases(400); s[[7, 100, 101, 399]] = [ord("N"), ord("a"), ord("c"), ord("n")]
    add("bases outside ACGT", s, np.ones(395))
    seq_len = np.array([len(r[0]) for r in reads], np.int32)
    seq_off = np.zeros(len(reads), np.int64); seq_off[1:] = np.cumsum(seq_len[:-1] + 3)          # reads need not touch
    arena = np.zeros(int(seq_off[-1] + seq_len[-1]) + 8, np.uint8)
    for o, r in zip(seq_off, reads):
        arena[o:o + len(r[0])] = r[0]
    event_off = np.zeros(len(reads) + 1, np.int64); np.cumsum([len(r[1]) for r in reads], out=event_off[1:])
    pairs, n_pairs = np.zeros(2 * int(event_off[-1]), PAIR_DTYPE), np.array([len(r[2]) for r in reads], np.int32)
    for o, r in zip(event_off, reads):
        assert len(r[2]) <= 2 * len(r[1])
        pairs[2 * o:2 * o + len(r[2])] = np.ascontiguousarray(r[2]).view(PAIR_DTYPE).reshape(-1)
    rs = AbeaReadSet(seq_off, seq_len, arena, event_off, np.concatenate([r[1] for r in reads]), np.full(len(reads), 1.0, np.float32),
                     np.full(len(reads), 0.5, np.float32), model)
    return rs, pairs, n_pairs, names


def edge_record_set():
    """The hand-made batch of the record tests -> dict(cigar_off, cigar, pos, rc, seq_off, seq_len, map, names): every CIGAR
    operation on both strands, clips that put aligned bases at read_pos 5 / 6 and len - 7 / len - 6, maps with holes of more
    than 1 000 k-mers, an all -1 map and records of one pair."""
    from genomicsbench_amd.datagen import bam_cigar
    rng = np.random.default_rng(4711)
    reads, names = [], []

    def dense_map(n, p=0.7):
        has = rng.random(n - 5) < p
        start = np.cumsum(rng.integers(1, 4, n - 5))
        m = np.where(has[:, None], np.stack([start, start + 1], 1), -1).astype(np.int32)
        return m

    def add(name, n, ops, m, pos=1000):
        for rc in (0, 1):
            reads.append((n, bam_cigar(ops), m, pos + 17 * rc, rc))
            names.append("%s, rc %d" % (name, rc))

    add("every operation", 400, [(7, "H"), (9, "S"), (50, "M"), (3, "I"), (40, "="), (5, "D"), (2, "X"), (100, "M"), (1, "D"), (1, "I"), (180, "M"),
                                 (15, "S"), (4, "H")], dense_map(400))
    add("soft clip of 5", 60, [(5, "S"), (55, "M")], dense_map(60, 0.9))
    add("soft clip of 6", 60, [(6, "S"), (54, "M")], dense_map(60, 0.9))
    add("all match", 60, [(60, "=")], dense_map(60, 0.9))
    add("ends at len - 7", 60, [(54, "M"), (6, "S")], dense_map(60, 0.9))
    add("ends at len - 6", 60, [(55, "M"), (5, "S")], dense_map(60, 0.9))
    add("more than 64 operations", 700, [(3, "M"), (1, "I"), (2, "="), (1, "D")] * 100 + [(100, "S")], dense_map(700, 0.5))
    m = np.full((2995, 2), -1, np.int32); m[:100] = np.arange(100)[:, None] * 2 + [0, 1]; m[2500:2600] = 1000 + np.arange(100)[:, None] * 2 + [0, 1]
    add("holes of more than 1000 k-mers", 3000, [(3000, "M")], m)
    add("no k-mer has events", 500, [(500, "M")], np.full((495, 2), -1, np.int32))
    add("one pair", 13, [(13, "M")], dense_map(13, 1.0))
    add("one pair without an event", 13, [(13, "M")], np.full((8, 2), -1, np.int32))
    add("no pair", 12, [(12, "M")], dense_map(12, 1.0))
    add("six bases", 6, [(6, "M")], dense_map(6, 1.0))
    add("no operation", 50, [], dense_map(50))
    add("aligned bases behind the read's end", 40, [(30, "S"), (20, "I"), (10, "M")], dense_map(40, 1.0))
    seq_len = np.array([r[0] for r in reads], np.int32)
    seq_off = np.zeros(len(reads), np.int64); seq_off[1:] = np.cumsum(seq_len[:-1] + 1)
    map_ = np.full((int(seq_off[-1] + seq_len[-1]) + 4, 2), -5, np.int32)
    for o, r in zip(seq_off, reads):
        map_[o:o + len(r[2])] = r[2]
    cigar_off = np.zeros(len(reads) + 1, np.int64); np.cumsum([len(r[1]) for r in reads], out=cigar_off[1:])
    return dict(cigar_off=cigar_off, cigar=np.concatenate([r[1] for r in reads]), pos=np.array([r[3] for r in reads], np.int32),
                rc=np.array([r[4] for r in reads], np.uint8), seq_off=seq_off, seq_len=seq_len, map=map_, names=names)
