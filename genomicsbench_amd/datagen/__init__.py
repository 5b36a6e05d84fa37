"""Seeded synthetic datasets in the reference input shapes.  Tooling only."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(os.path.dirname(_HERE), "libgbx_datagen.so")
_lib = None


def _L():
    global _lib
    if _lib is None:
        from ..build import build_datagen
        build_datagen()                      # no-op when the library is newer than datagen.c
        _lib = C.CDLL(_LIB)
        vp, i64, u64 = C.c_void_p, C.c_int64, C.c_uint64
        _lib.gbx_gen_bsw_lengths.argtypes = [u64, i64, i64, vp, vp, vp]
        _lib.gbx_gen_bsw_lengths.restype = None
        _lib.gbx_gen_bsw_fill.argtypes = [u64, i64, i64, vp, vp, vp, vp, vp, vp]
        _lib.gbx_gen_bsw_fill.restype = None
        _lib.gbx_gen_chain_count.argtypes = [u64, i64]
        _lib.gbx_gen_chain_count.restype = i64
        _lib.gbx_gen_chain_fill.argtypes = [u64, i64, i64, vp, vp]
        _lib.gbx_gen_chain_fill.restype = None
        _lib.gbx_gen_phmm_batch.argtypes = [u64, i64, C.c_int] + [vp] * 10
        _lib.gbx_gen_phmm_batch.restype = None
        _lib.gbx_gen_poa_window.argtypes = [u64, i64, C.c_int, vp, vp, vp]
        _lib.gbx_gen_poa_window.restype = None
        _lib.gbx_gen_chain_counts_many.argtypes = [u64, i64, i64, vp]
        _lib.gbx_gen_chain_fill_many.argtypes = [u64, i64, i64, vp, vp, vp]
        _lib.gbx_gen_chain_fill_real_many.argtypes = [u64, i64, i64, vp, vp, vp]
        _lib.gbx_gen_phmm_counts_many.argtypes = [u64, i64, i64, vp, vp]
        _lib.gbx_gen_phmm_lengths_many.argtypes = [u64, i64, i64, vp, vp, vp, vp]
        _lib.gbx_gen_phmm_fill_many.argtypes = [u64, i64, i64] + [vp] * 10
        _lib.gbx_gen_poa_counts_many.argtypes = [u64, i64, i64, vp]
        _lib.gbx_gen_poa_many.argtypes = [u64, i64, i64, C.c_int, vp, vp, vp, vp]
        _lib.gbx_gen_abea_model.argtypes = [u64, vp, vp]
        _lib.gbx_gen_abea_counts_many.argtypes = [u64, i64, i64, vp, vp]
        _lib.gbx_gen_abea_fill_many.argtypes = [u64, i64, i64] + [vp] * 8
        _lib.gbx_gen_abea_raw_counts_many.argtypes = [u64, i64, i64] + [vp] * 4
        _lib.gbx_gen_abea_raw_fill_many.argtypes = [u64, i64, i64] + [vp] * 12
        _lib.gbx_gen_abea_raw_counts_many.restype = _lib.gbx_gen_abea_raw_fill_many.restype = None
        _lib.gbx_gen_abea_kmer_events_many.argtypes = [u64, i64, i64, vp, vp]
        _lib.gbx_gen_abea_kmer_events_many.restype = None
        _lib.gbx_gen_fmi_genome.argtypes = [u64, i64, vp]
        _lib.gbx_gen_fmi_reads.argtypes = [u64, i64, i64, vp, i64, C.c_int32, vp]
        for f in ("abea_model", "abea_counts_many", "abea_fill_many", "fmi_genome", "fmi_reads"):
            getattr(_lib, "gbx_gen_" + f).restype = None
        for f in ("chain_counts_many", "chain_fill_many", "chain_fill_real_many", "phmm_counts_many", "phmm_lengths_many", "phmm_fill_many",
                  "poa_counts_many", "poa_many"):
            getattr(_lib, "gbx_gen_" + f).restype = None
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def gen_bsw(n_pairs, seed, first=0):
    """bsw 'small' = (100_000, seed 1001); 'large' = (2_000_000, seed 1002).  Returns a BswBatch."""
    from ..bsw import BswBatch
    L = _L()
    len1 = np.zeros(n_pairs, dtype=np.int32)
    len2 = np.zeros(n_pairs, dtype=np.int32)
    h0 = np.zeros(n_pairs, dtype=np.int32)
    L.gbx_gen_bsw_lengths(seed, first, n_pairs, _p(len1), _p(len2), _p(h0))
    a1 = (len1.astype(np.int64) + 3) & ~3
    a2 = (len2.astype(np.int64) + 3) & ~3
    idr = np.concatenate([[0], np.cumsum(a1)[:-1]]).astype(np.int64) if n_pairs else np.zeros(0, np.int64)
    idq = np.concatenate([[0], np.cumsum(a2)[:-1]]).astype(np.int64) if n_pairs else np.zeros(0, np.int64)
    ref = np.zeros(int(a1.sum()) + 4, dtype=np.uint8)
    qer = np.zeros(int(a2.sum()) + 4, dtype=np.uint8)
    L.gbx_gen_bsw_fill(seed, first, n_pairs, _p(len1), _p(len2), _p(idr), _p(idq), _p(ref), _p(qer))
    return BswBatch(ref, qer, idr, idq, len1, len2, h0)


def write_bsw_pairs_fast(path, b):
    """The reference's bsw input file for a BswBatch (same bytes as io.write_bsw_pairs, written by the C library)."""
    L = _L()
    L.gbx_write_bsw_pairs.restype = C.c_int64
    got = L.gbx_write_bsw_pairs(str(path).encode(), C.c_int64(b.n), _p(b.ref), _p(b.idr), _p(b.len1), _p(b.qer), _p(b.idq), _p(b.len2), _p(b.h0))
    if got < 0:
        raise OSError("cannot write %s" % path)
    return got


def gen_chain(n_calls, seed, first=0, n_override=None, realistic=False):
    """chain 'large' = (10_000, seed 2001).  Returns (anchor_off, ax, ay, hdr).  realistic=True: the same call sizes with
    minimap2's structure inside a call (both strands, six reference ids in the upper x word, repeat copies, isolated
    hits: datagen.c gbx_gen_chain_fill_real)."""
    from .._native import CHAIN_CALL_DTYPE
    L = _L()
    if n_override is None:
        counts = np.zeros(n_calls, dtype=np.int64)
        L.gbx_gen_chain_counts_many(seed, first, n_calls, _p(counts))
    else:
        counts = np.array([n_override[c] for c in range(n_calls)], dtype=np.int64)
    off = np.zeros(n_calls + 1, dtype=np.int64)
    np.cumsum(counts, out=off[1:])
    ax = np.zeros(int(off[-1]), dtype=np.uint64)
    ay = np.zeros(int(off[-1]), dtype=np.uint64)
    (L.gbx_gen_chain_fill_real_many if realistic else L.gbx_gen_chain_fill_many)(seed, first, n_calls, _p(off), _p(ax), _p(ay))
    hdr = np.zeros(n_calls, dtype=CHAIN_CALL_DTYPE)
    hdr["avg_qspan"] = 15.0
    hdr["max_dist_x"] = 5000
    hdr["max_dist_y"] = 5000
    hdr["bw"] = 500
    hdr["n_segs"] = 1
    return off, ax, ay, hdr


def gen_phmm(n_batches, seed, first=0):
    """phmm 'large' = (20_000 batches, seed 3001).  Returns a PhmmBatchSet (flat arenas + pair list)."""
    from ..phmm import PhmmBatchSet
    L = _L()
    nr = np.zeros(n_batches, dtype=np.int32)
    nh = np.zeros(n_batches, dtype=np.int32)
    L.gbx_gen_phmm_counts_many(seed, first, n_batches, _p(nr), _p(nh))
    roff = np.zeros(n_batches + 1, dtype=np.int64); np.cumsum(nr, out=roff[1:])
    hoff = np.zeros(n_batches + 1, dtype=np.int64); np.cumsum(nh, out=hoff[1:])
    read_len = np.zeros(int(roff[-1]), dtype=np.int32)
    hap_len = np.zeros(int(hoff[-1]), dtype=np.int32)
    L.gbx_gen_phmm_lengths_many(seed, first, n_batches, _p(roff), _p(hoff), _p(read_len), _p(hap_len))
    read_off = np.zeros(len(read_len) + 1, dtype=np.int64); np.cumsum(read_len, out=read_off[1:])
    hap_off = np.zeros(len(hap_len) + 1, dtype=np.int64); np.cumsum(hap_len, out=hap_off[1:])
    rs, q, qi, qd, qc = (np.zeros(int(read_off[-1]) + 8, dtype=np.uint8) for _ in range(5))
    hap = np.zeros(int(hap_off[-1]) + 8, dtype=np.uint8)
    L.gbx_gen_phmm_fill_many(seed, first, n_batches, _p(roff), _p(hoff), _p(read_off), _p(hap_off), _p(rs), _p(q),
                             _p(qi), _p(qd), _p(qc), _p(hap))
    return PhmmBatchSet(nr, nh, read_off[:-1].copy(), read_len, rs, q, qi, qd, qc, hap_off[:-1].copy(), hap_len, hap)


def gen_poa(n_windows, seed, first=0):
    """poa 'large' = (6_000 windows, seed 4001).  Returns a PoaWindowSet."""
    from ..poa import PoaWindowSet
    L = _L()
    nr = np.zeros(n_windows, dtype=np.int32)
    L.gbx_gen_poa_counts_many(seed, first, n_windows, _p(nr))
    wf = np.zeros(n_windows + 1, dtype=np.int64); np.cumsum(nr, out=wf[1:])
    lens = np.zeros(int(wf[-1]), dtype=np.int32)
    off = np.zeros(len(lens) + 1, dtype=np.int64)
    L.gbx_gen_poa_many(seed, first, n_windows, 1, _p(wf), _p(lens), _p(off), None)
    np.cumsum(lens, out=off[1:])
    arena = np.zeros(int(off[-1]) + 8, dtype=np.uint8)
    L.gbx_gen_poa_many(seed, first, n_windows, 2, _p(wf), _p(lens), _p(off), _p(arena))
    return PoaWindowSet(wf, off[:-1].copy(), lens, arena)


def gen_abea(n_reads, seed, first=0):
    """abea 'large' = (10000 reads, seed 5001), the read count of the reference's large input.  Returns an AbeaReadSet (synthetic pore model, reads, events, scalings)."""
    from ..abea import AbeaReadSet, make_model
    L = _L()
    lm, ls = np.zeros(4096, np.float32), np.zeros(4096, np.float32)
    L.gbx_gen_abea_model(seed, _p(lm), _p(ls))
    seq_len = np.zeros(n_reads, dtype=np.int32)
    n_ev = np.zeros(n_reads, dtype=np.int64)
    L.gbx_gen_abea_counts_many(seed, first, n_reads, _p(seq_len), _p(n_ev))
    seq_off = np.zeros(n_reads + 1, dtype=np.int64); np.cumsum(seq_len, out=seq_off[1:])
    event_off = np.zeros(n_reads + 1, dtype=np.int64); np.cumsum(n_ev, out=event_off[1:])
    seq = np.zeros(int(seq_off[-1]) + 8, dtype=np.uint8)
    ev = np.zeros(int(event_off[-1]) + 4, dtype=np.float32)
    scale, shift = np.zeros(n_reads, np.float32), np.zeros(n_reads, np.float32)
    L.gbx_gen_abea_fill_many(seed, first, n_reads, _p(lm), _p(ls), _p(seq_off), _p(event_off), _p(seq), _p(ev), _p(scale), _p(shift))
    return AbeaReadSet(seq_off[:-1].copy(), seq_len, seq, event_off, ev[:int(event_off[-1])], scale, shift, make_model(lm, ls))


def gen_abea_raw(n_reads, seed, first=0):
    """Raw signal for the reads of gen_abea(n_reads, seed, first): an AbeaSignalSet (int16 ADC counts, range / digitisation /
    offset, the reads' bases and the pore model) with the generator's true scalings in .true_scale / .true_shift.  Some reads
    fail the exactness predicate of the event kernels and some have no events (datagen.c)."""
    from ..abea_signal import AbeaSignalSet
    rs = gen_abea(n_reads, seed, first)
    L = _L()
    lm, ls = np.ascontiguousarray(rs.model["level_mean"]), np.ascontiguousarray(rs.model["level_stdv"])
    ns = np.zeros(n_reads, dtype=np.int64)
    L.gbx_gen_abea_raw_counts_many(seed, first, n_reads, _p(rs.seq_off), _p(rs.seq_len), _p(rs.seq_arena), _p(ns))
    raw_off = np.zeros(n_reads + 1, dtype=np.int64); np.cumsum(ns, out=raw_off[1:])
    raw = np.zeros(int(raw_off[-1]) + 8, dtype=np.int16)
    rg, dg, of = (np.zeros(n_reads, np.float32) for _ in range(3))
    L.gbx_gen_abea_raw_fill_many(seed, first, n_reads, _p(rs.seq_off), _p(rs.seq_len), _p(rs.seq_arena), _p(lm), _p(ls), _p(rs.scale),
                                 _p(rs.shift), _p(raw_off), _p(raw), _p(rg), _p(dg), _p(of))
    ss = AbeaSignalSet(raw[:int(raw_off[-1])], raw_off, rg, dg, of, rs.seq_off, rs.seq_len, rs.seq_arena, rs.model)
    ss.true_scale, ss.true_shift = rs.scale, rs.shift
    return ss


def _mix64(x):
    """splitmix64 finaliser on uint64 arrays: the seeded draws of gen_abea_meth that need no stream"""
    x = (np.asarray(x, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15))
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def _unif(seed, salt, idx):
    with np.errstate(over="ignore"):
        h = _mix64(_mix64(np.uint64(seed) * np.uint64(0x100000001B3) + np.uint64(salt)) + np.asarray(idx, dtype=np.uint64))
    return (h >> np.uint64(11)).astype(np.float64) / float(1 << 53)


def gen_abea_cpg_model(rs_model, seed):
    """Seeded synthetic CpG model over A < C < G < M < T: a k-mer without M has the level of gen_abea's model, one with M
    that of its C-for-M k-mer moved by U[-4, 4] pA (a draw per k-mer), the same stdv.  The reference's table is not used."""
    from ..abea_meth import NMODEL_CPG, make_cpg_model
    r = np.arange(NMODEL_CPG)
    digits = np.stack([(r // 5 ** (5 - i)) % 5 for i in range(6)], axis=1)        # first base most significant
    has_m = (digits == 3).any(axis=1)
    four = np.array([0, 1, 2, 1, 3])[digits]                                      # M reads as C
    r4 = (four * (4 ** np.arange(5, -1, -1))).sum(axis=1)
    lm = rs_model["level_mean"][r4].astype(np.float64) + np.where(has_m, 8.0 * _unif(seed, 0xC96, r) - 4.0, 0.0)
    return make_cpg_model(lm.astype(np.float32), rs_model["level_stdv"][r4])


def gen_abea_meth(n_reads, seed, first=0):
    """Reads as f5c call-methylation holds them behind align(), for the reads of gen_abea(n_reads, seed, first): an
    AbeaMethReadSet.  One read in four is rc: its reference segment is the reverse complement of its bases and its events
    run against the reference.  The read's own bases are the reference segment (an all-match alignment), starting at a
    seeded ref_start_pos; the event-alignment record is what get_event_alignment_record (meth.c:124-185) gives for the
    generator's own base-to-event map: per reference position 6 <= p < len - 6 the first event of the nearest k-mer at or
    before it (else after it) that has events.  var ~ U[0.9, 1.3], events_per_base = events / k-mers (at least 1.05).
    Uniform bases put a CpG every 16 bases: groups of one site (16 k-mers) dominate and chains up to the 200-base span occur."""
    from ..abea_meth import AbeaMethReadSet
    from ..abea import PAIR_DTYPE
    rs = gen_abea(n_reads, seed, first)
    L = _L()
    nk = rs.seq_len.astype(np.int64) - 5
    kmer_off = np.zeros(n_reads + 1, np.int64); np.cumsum(nk, out=kmer_off[1:])
    kcount = np.zeros(int(kmer_off[-1]) + 1, np.int32)
    L.gbx_gen_abea_kmer_events_many(seed, first, n_reads, _p(kmer_off), _p(kcount))
    ridx = np.arange(first, first + n_reads)
    rc = (_unif(seed, 0x5C, ridx) < 0.25).astype(np.uint8)
    ref_start_pos = (1000 + 100000 * _unif(seed, 0x57A, ridx)).astype(np.int32)
    var = (0.9 + 0.4 * _unif(seed, 0x7A5, ridx)).astype(np.float32)
    log_var = np.log(var.astype(np.float64)).astype(np.float32)
    n_ev = rs.n_events
    epb = np.maximum(n_ev / nk.astype(np.float64), 1.05)
    comp = np.zeros(256, np.uint8); comp[:] = ord("T")
    for a, b in zip(b"ACGT", b"TGCA"):
        comp[a] = b
    ref = np.zeros(int(rs.seq_len.sum()) + 8, np.uint8)
    ref_off = np.zeros(n_reads, np.int64)
    recs, rec_off, o = [], np.zeros(n_reads + 1, np.int64), 0
    for r in range(n_reads):
        n = int(rs.seq_len[r])
        bases = rs.seq_arena[rs.seq_off[r]:rs.seq_off[r] + n]
        ref_off[r] = o
        ref[o:o + n] = comp[bases[::-1]] if rc[r] else bases
        o += n
        kc = kcount[kmer_off[r]:kmer_off[r + 1]]
        firstev = np.cumsum(kc) - kc
        has = kc > 0
        rec_off[r + 1] = rec_off[r]
        if not has.any() or n < 13:
            continue
        at = np.where(has, np.arange(len(kc)), -1)
        before = np.maximum.accumulate(at)
        after = np.where(has, np.arange(len(kc)), len(kc))[::-1]
        after = np.minimum.accumulate(after)[::-1]
        near = np.where(before >= 0, before, after)
        p = np.arange(6, n - 6)
        kpos = n - p - 6 if rc[r] else p
        e = firstev[near[kpos]]
        if len(e) == 0 or e[0] == e[-1]:                                        # a degenerate alignment is discarded (meth.c:173-177)
            continue
        a = np.zeros(len(p), PAIR_DTYPE)
        a["ref_pos"], a["read_pos"] = ref_start_pos[r] + p, e
        recs.append(a)
        rec_off[r + 1] += len(a)
    rec = np.concatenate(recs) if recs else np.zeros(0, PAIR_DTYPE)
    ms = AbeaMethReadSet(rs, var, log_var, epb, rc, ref_off, rs.seq_len, ref[:o], ref_start_pos, rec_off, rec, gen_abea_cpg_model(rs.model, seed))
    ms.kmer_off, ms.kmer_events = kmer_off, kcount[:int(kmer_off[-1])]
    return ms


def bam_cigar(ops):
    """[(length, op letter)] -> the BAM encoding, len << 4 | code with MIDNSHP=X as 0..8"""
    return np.array([(int(n) << 4) | "MIDNSHP=X".index(o) for n, o in ops], dtype=np.uint32)


def gen_abea_cigars(ss, seed, first=0):
    """Alignments for the reads of gen_abea_raw / gen_abea(n_reads, seed, first), as call-methylation reads them from a BAM: per
    read a CIGAR (hard and soft clips at either end, between them blocks of M or = separated by an insertion, a deletion
    or a run of X), pos, rc (one read in four; the CIGAR then describes the reverse complement of the bases) and the
    reference segment derived from the read through the CIGAR: = and M copy the read's bases (one M base in 50 is changed),
    X changes them, D draws reference bases, I, S and H leave none.  -> dict(cigar_off, cigar, pos, rc, ref_off, ref_len,
    ref_arena, cpg_model)."""
    n_reads = ss.n_reads
    ridx = np.arange(first, first + n_reads)
    rc = (_unif(seed, 0x5C, ridx) < 0.25).astype(np.uint8)
    pos = (1000 + 100000 * _unif(seed, 0x57A, ridx)).astype(np.int32)
    comp = np.zeros(256, np.uint8); comp[:] = ord("T")
    for a, b in zip(b"ACGT", b"TGCA"):
        comp[a] = b
    other = np.zeros(256, np.uint8); other[:] = ord("C")               # a base that differs from the read's
    for a, b in zip(b"ACGT", b"CGTA"):
        other[a] = b
    acgt = np.frombuffer(b"ACGT", np.uint8)
    cigars, refs = [], []
    for r in range(n_reads):
        rng = np.random.default_rng([int(seed), 0xC16A, int(first) + r])
        n = int(ss.seq_len[r])
        q = ss.seq_arena[ss.seq_off[r]:ss.seq_off[r] + n]
        q = comp[q[::-1]] if rc[r] else q
        s0, s1 = (int(rng.integers(0, min(24, n // 8) + 1)) for _ in range(2))
        ops, ref, i, end = [], [], s0, n - s1
        if rng.random() < 0.5:
            ops.append((int(rng.integers(1, 30)), "H"))
        if s0:
            ops.append((s0, "S"))
        while i < end:
            m = min(int(rng.integers(8, 90)), end - i)
            kind = "=" if rng.random() < 0.4 else "M"
            seg = q[i:i + m].copy()
            if kind == "M":
                hit = rng.random(m) < 0.02
                seg[hit] = other[seg[hit]]
            ops.append((m, kind)); ref.append(seg); i += m
            if i >= end:
                break
            e, k = rng.random(), min(int(rng.integers(1, 4)), end - i)
            if e < 0.35:
                ops.append((k, "I")); i += k
            elif e < 0.7:
                ops.append((k, "D")); ref.append(acgt[rng.integers(0, 4, k)])
            else:
                ops.append((k, "X")); ref.append(other[q[i:i + k]]); i += k
        if s1:
            ops.append((s1, "S"))
        if rng.random() < 0.5:
            ops.append((int(rng.integers(1, 30)), "H"))
        cigars.append(bam_cigar(ops))
        refs.append(np.concatenate(ref) if ref else np.zeros(0, np.uint8))
    cigar_off = np.zeros(n_reads + 1, np.int64); np.cumsum([len(c) for c in cigars], out=cigar_off[1:])
    ref_len = np.array([len(x) for x in refs], np.int32)
    ref_off = np.zeros(n_reads, np.int64); ref_off[1:] = np.cumsum(ref_len[:-1])
    return dict(cigar_off=cigar_off, cigar=np.concatenate(cigars + [np.zeros(0, np.uint32)]), pos=pos, rc=rc, ref_off=ref_off, ref_len=ref_len,
                ref_arena=np.concatenate(refs + [np.zeros(8, np.uint8)]), cpg_model=gen_abea_cpg_model(ss.model, seed))


def gen_fmi_genome(length, seed):
    """Synthetic genome (one strand, base codes 0..3) with repeat families and low-complexity runs."""
    L = _L()
    ref = np.zeros(int(length), dtype=np.uint8)
    L.gbx_gen_fmi_genome(seed, int(length), _p(ref))
    return ref


def gen_fmi_reads(ref, n_reads, seed, first=0, read_len=151):
    """fmi reads: 151-bp samples of the genome (either strand, 1 % errors, a few N), the reference's fixed-stride layout."""
    from ..fmi import FmiReadSet
    L = _L()
    enc = np.zeros((int(n_reads), int(read_len)), dtype=np.uint8)
    L.gbx_gen_fmi_reads(seed, first, int(n_reads), _p(ref), len(ref), int(read_len), _p(enc))
    return FmiReadSet.fixed(enc)


KMER_PRESETS = {
    # the reference's inputs: Loman_E.coli_MAP006-1_2D_50x.fasta ('large', ~230 Mbp) and its first 1000 reads ('small')
    "small": dict(genome_len=4_600_000, coverage=None, n_reads=1000, seed=7001),
    "large": dict(genome_len=4_600_000, coverage=50.0, n_reads=None, seed=7002),
}


def gen_kmer_reads(genome_len, coverage, seed, n_reads=None, mean_len=9000, sub=0.06, ins=0.03, dele=0.03, repeat_copies=8,
                   repeat_len=3000, n_runs=4, short_frac=0.05):
    """Long noisy reads in the shape of kmer-cnt's nanopore input, deterministic in `seed`.  Returns [(name, ASCII bytes)].
    The genome carries `repeat_copies` copies of one `repeat_len` segment (k-mers seen hundreds of times) and a 200 bp
    homopolymer run.  Read lengths are log-normal around mean_len, clipped to 1..40 kbp, with `short_frac` of the reads
    drawn from 1..5000 bp (the reference's filter drops them); each read comes from either strand with about
    sub + ins + dele errors per base; `n_runs` reads carry a run of N or IUPAC codes.  n_reads, when given, overrides
    coverage."""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 4, genome_len, dtype=np.uint8)
    if repeat_copies > 0 and repeat_len * (repeat_copies + 1) < genome_len:
        rep = g[:repeat_len].copy()
        for s in rng.choice(np.arange(1, genome_len // repeat_len - 1), repeat_copies, replace=False):
            g[s * repeat_len:(s + 1) * repeat_len] = rep
    if genome_len > 1000:
        h = int(rng.integers(0, genome_len - 200))
        g[h:h + 200] = 0
    if n_reads is None:
        n_reads = max(1, int(genome_len * coverage / mean_len))
    sigma = 0.6
    lens = np.exp(rng.normal(np.log(mean_len) - sigma * sigma / 2, sigma, n_reads)).astype(np.int64)
    short = rng.random(n_reads) < short_frac
    lens[short] = rng.integers(1, 5001, int(short.sum()))
    lens = np.clip(lens, 1, min(40000, genome_len))
    runs = set(rng.choice(n_reads, min(n_runs, n_reads), replace=False).tolist())
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    out = []
    for r in range(n_reads):
        L = int(lens[r])
        st = int(rng.integers(0, genome_len - L + 1))
        s = g[st:st + L]
        if rng.random() < 0.5:
            s = 3 - s[::-1]
        u = rng.random(L)
        keep = u >= dele                                             # deletions
        sb = (u >= dele) & (u < dele + sub)
        s = np.where(sb, (s + rng.integers(1, 4, L, dtype=np.uint8)) % 4, s).astype(np.uint8)
        insr = (u >= dele + sub) & (u < dele + sub + ins)
        s = s[keep]
        insr = insr[keep]
        if insr.any():
            at = np.flatnonzero(insr) + 1
            s = np.insert(s, at, rng.integers(0, 4, at.size, dtype=np.uint8))
        txt = acgt[s]
        if r in runs and txt.size > 20:
            a = int(rng.integers(0, txt.size - 10))
            txt = txt.copy()
            txt[a:a + 10] = np.frombuffer(b"NNNNRYKMSW"[:10], dtype=np.uint8)
        out.append(("read_%d" % r, txt.tobytes()))
    return out


def gen_kmer_preset(name):
    p = KMER_PRESETS[name]
    return gen_kmer_reads(p["genome_len"], p["coverage"], p["seed"], n_reads=p["n_reads"])


def write_fasta(path, records, wrap=0, fastq=False):
    """records: [(name, ASCII bytes)].  wrap > 0 breaks FASTA sequence lines every `wrap` characters; fastq writes
    4-line records with constant qualities."""
    with open(path, "wb") as f:
        for name, seq in records:
            if fastq:
                f.write(b"@%s\n%s\n+\n%s\n" % (name.encode(), seq, b"5" * len(seq)))
            elif wrap > 0:
                f.write(b">%s\n" % name.encode())
                for i in range(0, len(seq), wrap):
                    f.write(seq[i:i + wrap] + b"\n")
            else:
                f.write(b">%s\n%s\n" % (name.encode(), seq))


# ------------------------------------------------------------------------------------------------------------- pileup
PILEUP_PRESETS = {
    # the shape of the reference's S. aureus input (R/README: a ~2.8 Mb genome of ONT reads), scaled to 1.5 Mb at 40x
    "small": dict(contig_len=1_500_000, coverage=40, mean_len=8000, seed=81),
    # a scaled-down chr20: 12 Mb at 50x, 12 kb mean reads
    "large": dict(contig_len=12_000_000, coverage=50, mean_len=12000, seed=82),
}
PILEUP_DTYPES = ("r941", "r10")


def _homopolymer_runs(ref):
    """run length of the homopolymer each reference base belongs to"""
    change = np.flatnonzero(np.diff(ref.astype(np.int16)) != 0) + 1
    starts = np.concatenate(([0], change))
    lens = np.diff(np.concatenate((starts, [ref.size])))
    return np.repeat(lens, lens)


def _sim_read(rng, ref, hp, start, span):
    """One ONT-like read over ref[start:start+span]: substitutions, IUPAC N, deletions and insertions (both three times
    as likely inside homopolymers; an insertion there repeats the homopolymer's base) -> (cigar [(op, len)], nt16 codes)."""
    seg, h = ref[start:start + span], hp[start:start + span] > 1
    boost = np.where(h, 3.0, 1.0)
    dele = rng.random(span) < 0.02 * boost
    ins = np.where(rng.random(span) < 0.015 * boost, rng.geometric(0.5, span), 0)
    ins[-1] = 0
    dele[0] = dele[-1] = False
    base = seg.copy()
    sub = rng.random(span) < 0.03
    base[sub] = (base[sub] + rng.integers(1, 4, int(sub.sum()))) % 4
    base[rng.random(span) < 0.001] = 4                          # N
    slots = 1 + ins
    first = np.concatenate(([0], np.cumsum(slots)[:-1]))
    total = int(slots.sum())
    ops = np.full(total, 1, dtype=np.int8)                      # I
    ops[first] = np.where(dele, 2, 0)                           # D / M
    idx = np.repeat(np.arange(span), slots)                     # the reference base each slot follows
    ins_base = np.where(h[idx], seg[idx], rng.integers(0, 4, total))
    qb = np.where(ops == 0, base[idx], ins_base)
    keep = ops != 2
    codes = np.array([1, 2, 4, 8, 15], dtype=np.uint8)[qb[keep]]
    change = np.flatnonzero(np.diff(ops) != 0) + 1
    st = np.concatenate(([0], change))
    ln = np.diff(np.concatenate((st, [total])))
    cigar = list(zip(ops[st].tolist(), ln.tolist()))
    return cigar, codes


def _quals(rng, n):
    """qualities spread over the homopolymer strata 1..5 and a little above"""
    return np.minimum(1 + rng.geometric(0.35, n), 60).astype(np.uint8)


def _pileup_chunk(args):
    from .. import pileup as P
    seed, c0, ref, hp, starts, lens, dts = args
    rng = np.random.default_rng([seed, c0])
    nt = np.array([1, 2, 4, 8], dtype=np.uint8)
    filt = (0x4, 0x100, 0x200, 0x400, 0x800)
    out = []
    for i in range(starts.size):
        r = c0 + i
        span = int(min(lens[i], ref.size - starts[i]))
        rev = int(rng.random() < 0.5)
        cigar, codes = _sim_read(rng, ref, hp, int(starts[i]), span)
        lclip, rclip = (int(rng.integers(1, 200)) if rng.random() < 0.3 else 0), (int(rng.integers(1, 200)) if rng.random() < 0.3 else 0)
        if lclip:
            cigar = [(4, lclip)] + cigar
            codes = np.concatenate((nt[rng.integers(0, 4, lclip)], codes))
        if rclip:
            cigar = cigar + [(4, rclip)]
            codes = np.concatenate((codes, nt[rng.integers(0, 4, rclip)]))
        if rng.random() < 0.1:
            cigar = [(5, int(rng.integers(1, 500)))] + cigar
        if rng.random() < 0.1:
            cigar = cigar + [(5, int(rng.integers(1, 500)))]
        qual = np.full(codes.size, 0xFF, dtype=np.uint8) if rng.random() < 0.02 else _quals(rng, codes.size)
        flag, mapq = 0x10 * rev, int(rng.integers(1, 61))
        u = rng.random()
        if u < 0.05:
            flag |= filt[int(rng.integers(0, len(filt)))]
        elif u < 0.06:
            mapq = 0
        passes = not (flag & P.FILTER_FLAGS) and mapq >= 1
        dt = dts[int(rng.integers(0, len(dts)))]
        out.append((int(starts[i]), passes, ("read_%d" % r, 0, int(starts[i]), mapq, flag, cigar, codes, qual, dt)))
    return out


def gen_pileup_reads(contig_len, coverage, seed, mean_len=8000, adversarial=False, n_dtypes=2, missing_dt=0, contig_name="ctg1",
                     workers=1):
    """A random contig (with homopolymer runs) and ONT-like reads on it, both strands, soft and hard clips, IUPAC N,
    reads with missing qualities, filtered reads (every flag of the filter, mapq 0) and a few reads on a second contig,
    as raw BAM records in coordinate order.  Each read carries DT:Z (one of PILEUP_DTYPES[:n_dtypes]) unless it is one of
    the first `missing_dt` kept reads.  adversarial adds one read per CIGAR case of the contract.
    -> (contigs [(name, length)], records [bytes])."""
    from .. import pileup as P
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 4, contig_len, dtype=np.uint8)
    for a in rng.integers(0, max(1, contig_len - 12), contig_len // 60):         # homopolymer runs of 3..8
        ref[a:a + int(rng.integers(3, 9))] = ref[a]
    hp = _homopolymer_runs(ref)
    n_reads = max(1, int(contig_len * coverage / mean_len))
    lens = np.clip(rng.gamma(2.0, mean_len / 2.0, n_reads).astype(np.int64), 200, max(201, contig_len - 2))
    starts = np.sort(rng.integers(0, np.maximum(1, contig_len - lens)))
    contigs = [(contig_name, contig_len), ("ctg2", 50000)]
    dts = PILEUP_DTYPES[:max(1, n_dtypes)]
    # reads in chunks of 256, each with a generator of its own: the same records whatever the number of workers
    chunks = [(seed, c, ref, hp, starts[c:c + 256], lens[c:c + 256], dts) for c in range(0, n_reads, 256)]
    if workers > 1 and len(chunks) > 1:
        import multiprocessing as mp
        with mp.get_context("fork").Pool(workers) as pool:
            parts = pool.map(_pileup_chunk, chunks)
    else:
        parts = [_pileup_chunk(c) for c in chunks]
    recs = []
    kept = 0
    for part in parts:
        for pos, passes, rec_args in part:
            name, tid, pos_, mapq, flag, cigar, codes, qual, dt = rec_args
            tags = b"" if (passes and kept < missing_dt) else P.dt_tag(dt)
            kept += passes
            recs.append((pos, P.bam_record(name, tid, pos_, mapq, flag, cigar, codes, qual, tags)))
    nt = np.array([1, 2, 4, 8], dtype=np.uint8)
    if adversarial:
        for k, (cigar, pos) in enumerate(_adversarial_cigars(contig_len)):
            qlen = sum(ln for op, ln in cigar if op in (0, 1, 4, 7, 8))
            codes = nt[rng.integers(0, 4, qlen)]
            if k % 3 == 0 and qlen > 2:
                codes[1] = 15
            recs.append((pos, P.bam_record("adv_%d" % k, 0, pos, 30, 0x10 * (k & 1), cigar, codes, _quals(rng, qlen),
                                           P.dt_tag(dts[k % len(dts)]))))
    recs.sort(key=lambda x: x[0])
    other = []
    for r in range(20):                                    # the second contig: never in a pileup of the first
        pos = int(rng.integers(0, 40000))
        codes = nt[rng.integers(0, 4, 500)]
        other.append((pos, P.bam_record("other_%d" % r, 1, pos, 30, 0, [(0, 500)], codes, _quals(rng, 500), P.dt_tag(dts[0]))))
    other.sort(key=lambda x: x[0])
    return contigs, [b for _, b in recs] + [b for _, b in other]


def _adversarial_cigars(contig_len):
    """(cigar, pos) of every CIGAR case of the contract, at fixed places near the contig's start"""
    M, I, D, N, S, H, P, EQ, X = range(9)
    base = min(1000, max(0, contig_len // 4))
    cases = [
        [(M, 10), (I, 3), (D, 2), (M, 10)],                    # I then D
        [(M, 10), (D, 2), (I, 3), (M, 10)],                    # D then I: the D's last position carries +3
        [(M, 8), (N, 20), (M, 8)],                             # refskip
        [(M, 8), (N, 5), (I, 4), (M, 8)],                      # N then I
        [(EQ, 5), (X, 1), (EQ, 5), (I, 2), (X, 3)],            # = and X
        [(M, 6), (P, 2), (I, 3), (M, 6)],                      # P then I
        [(M, 6), (I, 2), (P, 1), (I, 3), (M, 6)],              # I, P, I: the first I decides
        [(M, 6), (P, 1), (I, 2), (P, 1), (I, 1), (M, 6)],      # P I P I: their sum
        [(I, 4), (M, 12)],                                     # leading I: never reported
        [(S, 5), (I, 3), (M, 12)],                             # leading S and I
        [(H, 7), (S, 2), (M, 12), (I, 5)],                     # trailing I: reported
        [(M, 12), (I, 2), (S, 4), (H, 3)],                     # trailing I then clips
        [(M, 9), (D, 1), (D, 2), (M, 9)],                      # D after D: no indel for the first D
        [(M, 3), (I, 40), (M, 3)],                             # a long insertion
        [(M, 5), (D, 3), (N, 4), (M, 5)],                      # D then N
    ]
    return [(c, base + 7 * k) for k, c in enumerate(cases)]


def gen_pileup_preset(name, adversarial=False, workers=1):
    p = PILEUP_PRESETS[name]
    return gen_pileup_reads(p["contig_len"], p["coverage"], p["seed"], p["mean_len"], adversarial=adversarial, workers=workers)


# ---------------------------------------------------------------------------------------------------------- dbg
# contig lengths: 'small' is for the GPU tests (the plain-Python restatement checks every window of it); 'large' gives about
# 0.75e9 edge occurrences inserted (1.01e9 slots, 16 000 windows) for scripts/time_dbg.py
DBG_PRESETS = {
    "small": dict(contig_len=20000, coverage=30, seed=91),
    "large": dict(contig_len=12000000, coverage=40, seed=92),
}
_ASCII_NT16 = {c: i for i, c in enumerate("=ACMGRSVTWYHKDBN")}


def _dbg_contig(rng, n, adversarial):
    """ACGT with homopolymers and tandem repeats; adversarial: lowercase and N runs, and one k-mer followed by six different
    bytes (a node with more than 4 successors in the reference alone)"""
    ref = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].copy()
    for _ in range(max(1, n // 4000)):
        at = int(rng.integers(0, max(1, n - 200)))
        if rng.random() < 0.5:
            ref[at:at + int(rng.integers(8, 40))] = ref[at]                                       # homopolymer
        else:
            unit = ref[at:at + int(rng.integers(2, 7))].copy()
            reps = int(rng.integers(6, 20))
            run = np.tile(unit, reps)[:max(0, min(len(unit) * reps, n - at))]
            ref[at:at + run.size] = run                                                            # tandem repeat
    if adversarial:
        for _ in range(max(1, n // 5000)):
            at = int(rng.integers(0, max(1, n - 300)))
            ref[at:at + int(rng.integers(20, 200))] += 32                                         # lowercase run (ACGT -> acgt)
            at = int(rng.integers(0, max(1, n - 100)))
            ref[at:at + int(rng.integers(1, 30))] = ord("N")
        at = n // 2                                                                # a homopolymer and a tandem repeat long
        ref[at:at + 30] = ord("A")                                                 # enough for self-loops and cycles at k = 15
        ref[at + 60:at + 60 + 48] = np.frombuffer(b"CAG" * 16, dtype=np.uint8)
        key = b"GATTACAGATTACAG"
        at = n // 3
        for j, nxt in enumerate(b"ACGTaR"):
            s = at + 40 * j
            if s + 16 < n:
                ref[s:s + 15] = np.frombuffer(key, dtype=np.uint8)
                ref[s + 15] = nxt
    return ref


def _dbg_donor(rng, ref):
    """the sampled haplotype: SNPs (1 in 1000) and short indels (1 in 5000), with a map donor index -> reference position"""
    n = ref.size
    snp = rng.random(n) < 0.001
    alt = ref.copy()
    alt[snp] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(snp.sum()))]
    ev = np.flatnonzero(rng.random(n) < 0.0002)
    pieces, pmap, last = [], [], 0
    for e in ev:
        pieces.append(alt[last:e]); pmap.append(np.arange(last, e))
        if rng.random() < 0.5:
            ins = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(rng.integers(1, 6)))]
            pieces.append(ins); pmap.append(np.full(ins.size, e))
            last = e
        else:
            last = min(n, e + int(rng.integers(1, 6)))
    pieces.append(alt[last:]); pmap.append(np.arange(last, n))
    return np.concatenate(pieces), np.concatenate(pmap)


def gen_dbg_reads(contig_len, coverage, seed, read_len=150, adversarial=False, contig_name="ctg1", deep=2000):
    """Illumina-like reads of at most read_len bases at `coverage` over a contig with SNPs and indels ->
    (contigs [(name, length)], BAM records in coordinate order (pileup.bam_record), the contig's FASTA bytes).
    adversarial=True adds: lowercase and N runs in the reference, IUPAC and '=' bases in reads, homopolymers and tandem
    repeats, a k-mer with six successors, qualities around 20, QC-fail records, unmapped records with a position, leading
    soft clips at the contig start (the uint32 wrap), reads shorter than k + 2, a stretch of windows with no reads and one
    window of `deep` extra reads (the capacity path)."""
    from ..pileup import bam_record
    rng = np.random.default_rng(seed)
    ref = _dbg_contig(rng, contig_len, adversarial)
    donor, dmap = _dbg_donor(rng, np.where(ref >= 97, ref - 32, ref).astype(np.uint8))
    n_reads = int(contig_len * coverage / read_len)
    starts = np.sort(rng.integers(0, max(1, donor.size - read_len), n_reads))
    if adversarial:
        gap0, gap1 = int(contig_len * 0.6), int(contig_len * 0.6) + 4000          # no reads start or end in here
        starts = starts[(dmap[np.minimum(starts + read_len, donor.size - 1)] < gap0) | (dmap[starts] >= gap1)]
        extra = np.full(deep, donor.size // 5)
        starts = np.sort(np.concatenate((starts, extra, [0, 2, 4])))
    enc = np.zeros(256, dtype=np.uint8)
    for c, v in _ASCII_NT16.items():
        enc[ord(c)] = v
        enc[ord(c.lower())] = v
    recs = []
    for i, st in enumerate(starts.tolist()):
        ln = read_len
        if adversarial and rng.random() < 0.03:
            ln = int(rng.integers(1, 18))                                         # shorter than k + 2
        seg = donor[st:st + ln].copy()
        ln = seg.size
        if ln == 0:
            continue
        err = rng.random(ln) < 0.004
        seg[err] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(err.sum()))]
        codes = enc[seg]
        if adversarial:
            iu = rng.random(ln) < 0.003
            codes[iu] = rng.choice(np.array([0, 3, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15], dtype=np.uint8), int(iu.sum()))
        if adversarial and rng.random() < 0.5:
            q = np.clip(rng.normal(23, 2, ln), 2, 41).astype(np.uint8)              # around min_qual
        else:
            q = np.clip(rng.normal(36, 3, ln) - np.linspace(0, 8, ln), 2, 41).astype(np.uint8)
            q[rng.random(ln) < 0.02] = 8
        pos = int(dmap[st])
        cigar = [(0, ln)]
        flag = 0x10 if rng.random() < 0.5 else 0
        if adversarial:
            u = rng.random()
            if u < 0.02:
                flag |= 0x200                                                      # QC fail
            elif u < 0.04:
                flag |= 0x4                                                        # unmapped, placed
                cigar = []
            if pos < 40 and ln > 12 and (pos < 8 or rng.random() < 0.7):
                cigar = [(4, 10), (0, ln - 10)]                                    # leading clip at the contig start: pos - 10 wraps
        recs.append((pos, bam_record("r%d" % i, 0, pos, 60, flag, cigar, codes, q)))
    recs.sort(key=lambda x: x[0])
    fasta = b">" + contig_name.encode() + b"\n" + b"\n".join(ref[i:i + 60].tobytes() for i in range(0, ref.size, 60)) + b"\n"
    return [(contig_name, contig_len)], [r for _, r in recs], fasta


def gen_dbg_preset(name, adversarial=False):
    p = DBG_PRESETS[name]
    return gen_dbg_reads(p["contig_len"], p["coverage"], p["seed"], adversarial=adversarial)
