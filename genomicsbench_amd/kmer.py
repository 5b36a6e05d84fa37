"""Host mirror of the reference kmer-cnt interface (R/benchmarks/kmer-cnt: SequenceContainer::loadFromFile and Flye's
KmerCounter::count, vertex_index.cpp:513-612).

``read_fasta`` parses FASTA (wrapped or not) and FASTQ as the reference does: only reads longer than ``min_read_len`` are
kept (sequence_container.cpp:102), and a character outside ``ACGTacgt`` turns itself and the rest of its 32-base chunk
into T (``encode``: what the reference's packing does with it on LP64).
``count_host`` / ``DeviceKmer`` call libgbx.so; all counting happens there on the GPU.
"""
import ctypes as C
import gzip
import os

import numpy as np

from . import _native as N

MAX_K = 17
STATS_FIELDS = ("n_positions", "n_distinct", "n_ge16", "max_count", "n_selected")

# ACGTacgt -> 0 1 2 3, everything else 255 (sequence.h:163-174)
_LUT = np.full(256, 255, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _LUT[_c] = _i
    _LUT[bytes([_c]).lower()[0]] = _i


class KmerParams(C.Structure):          # gbx_kmer_params
    _fields_ = [("k", C.c_int32), ("n_hist", C.c_int32), ("min_freq", C.c_uint32), ("max_freq", C.c_uint32)]


class KmerStats(C.Structure):           # gbx_kmer_stats
    _fields_ = [(f, C.c_int64) for f in STATS_FIELDS]


def encode(seq):
    """Base codes of one record's ASCII sequence as the reference stores it.  ACGTacgt -> 0 1 2 3.  Any other character
    makes itself and every later base of its 32-base chunk T (3): DnaSequence packs 32 bases into a 64-bit word by OR-ing
    dnaToId(c) << 2 (i % 32), and dnaToId of such a character is size_t(-1) (sequence.h:59-68,143-146), whose shift sets
    all the word's higher bits.  The "ACGT"[rand() % 4] replacement meant to prevent this (sequence_container.cpp:318-328)
    never runs on LP64: it compares that size_t(-1) with -1U, which is 2^32 - 1."""
    codes = _LUT[np.frombuffer(seq, dtype=np.uint8) if isinstance(seq, (bytes, bytearray)) else np.asarray(seq, dtype=np.uint8)]
    bad = codes == 255
    if bad.any():
        n = codes.size
        pad = np.zeros((n + 31) // 32 * 32, dtype=bool)
        pad[:n] = bad
        spill = np.logical_or.accumulate(pad.reshape(-1, 32), axis=1).reshape(-1)[:n]
        codes = np.where(spill, np.uint8(3), codes).astype(np.uint8)
    return codes


class KmerReadSet:
    """Reads as base codes 0..3, one per byte: read r = enc[read_off[r] ..+ read_len[r])."""

    def __init__(self, enc, read_off, read_len, names=None):
        self.enc = np.ascontiguousarray(enc, dtype=np.uint8)
        self.read_off = np.ascontiguousarray(read_off, dtype=np.int64)
        self.read_len = np.ascontiguousarray(read_len, dtype=np.int32)
        self.names = names

    @property
    def n_reads(self):
        return int(self.read_len.size)

    @property
    def n_bases(self):
        return int(self.read_len.astype(np.int64).sum())

    def n_positions(self, k):
        return int(np.maximum(self.read_len.astype(np.int64) - k, 0).sum())

    @classmethod
    def from_codes(cls, reads):
        """reads: a list of sequences of base codes 0..3 (numpy arrays or lists), packed back to back."""
        arrs = [np.asarray(r, dtype=np.uint8).reshape(-1) for r in reads]
        lens = np.array([a.size for a in arrs], dtype=np.int32)
        off = np.zeros(len(arrs), dtype=np.int64)
        if len(arrs) > 1:
            off[1:] = np.cumsum(lens[:-1], dtype=np.int64)
        enc = np.concatenate(arrs) if arrs else np.zeros(0, dtype=np.uint8)
        return cls(enc, off, lens)

    @classmethod
    def from_records(cls, records, min_read_len=5000):
        """records: (name, ASCII sequence as bytes or a uint8 array) in file order -> the reads longer than min_read_len
        (sequence_container.cpp:102), encoded as the reference stores them (encode)."""
        names, seqs = [], []
        for name, seq in records:
            if len(seq) > min_read_len:
                names.append(name)
                seqs.append(encode(seq))
        rs = cls.from_codes(seqs)
        rs.names = names
        return rs

    def checksum(self):
        """FNV-1a 64 over read_len (int32) and then the bases: what `kmer-cnt --parse-only` prints."""
        h = 1469598103934665603
        for b in (self.read_len.tobytes(), self._packed().tobytes()):
            h = _fnv1a(b, h)
        return "%016x" % h

    def _packed(self):
        if self.n_reads == 0:
            return np.zeros(0, dtype=np.uint8)
        return np.concatenate([self.enc[o:o + n] for o, n in zip(self.read_off.tolist(), self.read_len.tolist())])


def _fnv1a(data, h):
    prime, mask = 1099511628211, (1 << 64) - 1
    for v in bytes(data):
        h = ((h ^ v) * prime) & mask
    return h


def _open_text(path):
    with open(path, "rb") as f:
        magic = f.read(2)
    return gzip.open(path, "rb") if magic == b"\x1f\x8b" else open(path, "rb")


def is_fasta(path):
    """The reference's rule (sequence_container.cpp:23-48): by suffix, .gz ignored; .fasta / .fa or .fastq / .fq."""
    name = path[:-3] if path.endswith(".gz") else path
    suffix = name.rsplit(".", 1)[-1] if "." in os.path.basename(name) else ""
    if suffix in ("fasta", "fa"):
        return True
    if suffix in ("fastq", "fq"):
        return False
    raise ValueError("Can't identify input file type: %s" % path)


def parse_records(path):
    """[(name, ASCII sequence bytes)] of a FASTA (wrapped lines joined) or FASTQ file, in file order."""
    with _open_text(path) as f:
        lines = f.read().split(b"\n")
    recs = []
    if is_fasta(path):
        name, parts = None, []
        for ln in lines:
            if not ln:
                continue
            if ln.endswith(b"\r"):
                ln = ln[:-1]
            if ln[:1] == b">":
                if name is not None:
                    recs.append((name, b"".join(parts)))
                name, parts = ln[1:].split(None, 1)[0].decode() if ln[1:].strip() else "", []
            else:
                parts.append(ln)
        if name is not None:
            recs.append((name, b"".join(parts)))
    else:
        state, name = 0, None
        for ln in lines:
            if not ln:
                state = (state + 1) % 4
                continue
            if ln.endswith(b"\r"):
                ln = ln[:-1]
            if state == 0:
                if ln[:1] != b"@":
                    raise ValueError("Fastq format error in %s" % path)
                name = ln[1:].split(None, 1)[0].decode()
            elif state == 1:
                recs.append((name, ln))
            state = (state + 1) % 4
    return recs


def read_fasta(paths, min_read_len=5000):
    """One KmerReadSet from one or more FASTA / FASTQ files (a path, or a list of them, in order, as the reference's
    loadFromFile calls take them)."""
    if isinstance(paths, str):
        paths = [paths]
    recs = []
    for p in paths:
        recs.extend(parse_records(p))
    return KmerReadSet.from_records(recs, min_read_len)


def _params(k, n_hist, min_freq, max_freq):
    return KmerParams(int(k), int(n_hist), int(min_freq), int(max_freq))


def _stats_dict(st):
    return {f: int(getattr(st, f)) for f in STATS_FIELDS}


def count_host(reads, k, n_hist=256, min_freq=0, max_freq=0, sel_cap=None):
    """gbx_kmer_count_host -> (stats dict, hist int64[n_hist], kmers uint64[n], counts uint32[n]).  Without sel_cap the
    output starts at min(n_positions, 2^20) and is resized once to the needed count."""
    p = _params(k, n_hist, min_freq, max_freq)
    hist = np.zeros(max(n_hist, 0), dtype=np.int64)
    cap = int(sel_cap) if sel_cap is not None else (0 if min_freq == 0 else min(reads.n_positions(k), 1 << 20))
    st = KmerStats()
    for attempt in range(2):
        kmers = np.zeros(cap, dtype=np.uint64)
        counts = np.zeros(cap, dtype=np.uint32)
        rc = N.lib().gbx_kmer_count_host(C.byref(p), reads.n_reads, N.ptr(reads.enc), reads.enc.size, N.ptr(reads.read_off),
                                         N.ptr(reads.read_len), C.byref(st), N.ptr(hist) if n_hist else None, N.ptr(kmers),
                                         N.ptr(counts), cap)
        if rc == N.GBX_ERR_ARG and sel_cap is None and attempt == 0 and st.n_selected > cap:
            cap = int(st.n_selected)
            continue
        N.check(rc)
        break
    n = min(int(st.n_selected), cap)
    return _stats_dict(st), hist, kmers[:n], counts[:n]


class DeviceKmer:
    """Device-resident reads + outputs + workspace; run() = one gbx_kmer_count_device call on `stream`."""

    def __init__(self, reads, device, k, n_hist=256, min_freq=0, max_freq=0, sel_cap=0):
        import torch
        self.dev = torch.device(device)
        self.n_reads = reads.n_reads
        self.enc = torch.from_numpy(reads.enc if reads.enc.size else np.zeros(1, dtype=np.uint8)).to(self.dev)
        self.read_off = torch.from_numpy(reads.read_off).to(self.dev)
        self.read_len = torch.from_numpy(reads.read_len).to(self.dev)
        self.stats = torch.zeros(len(STATS_FIELDS), dtype=torch.int64, device=self.dev)
        self.set_params(k, n_hist, min_freq, max_freq, sel_cap)

    def set_params(self, k, n_hist=256, min_freq=0, max_freq=0, sel_cap=0):
        import torch
        self.params = _params(k, n_hist, min_freq, max_freq)
        self.n_hist, self.sel_cap = int(n_hist), int(sel_cap)
        self.hist = torch.zeros(max(self.n_hist, 1), dtype=torch.int64, device=self.dev)
        self.sel_kmer = torch.zeros(max(self.sel_cap, 1), dtype=torch.int64, device=self.dev)
        self.sel_count = torch.zeros(max(self.sel_cap, 1), dtype=torch.int32, device=self.dev)
        wb = N.lib().gbx_kmer_workspace_bytes(int(k), self.n_reads, self.n_hist)
        if wb == 0:
            raise ValueError("kmer: k = %d outside 1..%d" % (k, MAX_K))
        if getattr(self, "work", None) is None or self.work.numel() < wb:
            self.work = None
            self.work = torch.empty(wb, dtype=torch.uint8, device=self.dev)
        self.work_bytes = wb

    def run(self, stream=None):
        N.check(N.lib().gbx_kmer_count_device(C.byref(self.params), self.n_reads, self.enc.data_ptr(), self.read_off.data_ptr(),
                                              self.read_len.data_ptr(), self.stats.data_ptr(), self.hist.data_ptr(),
                                              self.sel_kmer.data_ptr(), self.sel_count.data_ptr(), self.sel_cap,
                                              self.work.data_ptr(), self.work_bytes, stream))

    def results(self):
        """-> (stats dict, hist, kmers, counts) as count_host returns them (the selection cut at sel_cap)."""
        st = dict(zip(STATS_FIELDS, (int(v) for v in self.stats.cpu().tolist())))
        n = max(0, min(st["n_selected"], self.sel_cap))
        hist = self.hist.cpu().numpy()[:self.n_hist].copy()
        return st, hist, self.sel_kmer[:n].cpu().numpy().view(np.uint64).copy(), self.sel_count[:n].cpu().numpy().view(np.uint32).copy()


def kmer_text(code, k):
    """ACGT text of a k-mer code (first base most significant)."""
    return "".join("ACGT"[(int(code) >> (2 * (k - 1 - i))) & 3] for i in range(k))
