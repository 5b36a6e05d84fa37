"""Host side of the dbg benchmark (R/benchmarks/dbg: Platypus's de Bruijn graph assembly of a BAM region).

``read_bam`` returns every record of a region in file order, as the reference's region iterator does (no filter), with the
reference's per-read refusals; it reuses pileup.py's BGZF/BAM reader.  ``read_fasta`` / ``fetch`` are the FASTA side
(no .fai).  ``make_windows`` applies the window and read-range rule through gbx_dbg_windows; ``build_host`` /
``graph_host`` / ``DeviceDbg`` call libgbx.so, where every graph is built on the GPU.
"""
import ctypes as C

import numpy as np

from . import _native as N
from . import pileup as P

NT16 = b"=ACMGRSVTWYHKDBN"
_NT16 = np.frombuffer(NT16, dtype=np.uint8)
STATS_FIELDS = ("n_nodes", "n_edges", "n_dropped", "n_occ", "weight_sum", "n_ref", "n_read", "n_both", "digest")
STATS_DTYPE = np.dtype([(f, "<i8") for f in STATS_FIELDS[:-1]] + [("digest", "<u8")])
NODE_DTYPE = np.dtype({"names": ["weight", "src", "first_edge", "position", "colours", "n_edges"],
                       "formats": ["<i8", "<i8", "<i8", "<i4", "u1", "u1"], "offsets": [0, 8, 16, 24, 28, 29], "itemsize": 32})
EDGE_DTYPE = np.dtype({"names": ["weight", "end"], "formats": ["<i8", "<i4"], "offsets": [0, 8], "itemsize": 16})
# the reference's limits (common.h: MAX_READNAME_LEN, MAX_READ_LEN, MAX_N_CIGAR)
MAX_READNAME_LEN, MAX_READ_LEN, MAX_N_CIGAR = 100, 151, 16


class DbgParams(C.Structure):              # gbx_dbg_params
    _fields_ = [("k", C.c_int32), ("min_qual", C.c_int32), ("region_size", C.c_int32), ("pad_", C.c_int32)]


class DbgReadsC(C.Structure):              # gbx_dbg_reads
    _fields_ = [("n_reads", C.c_int64), ("seq_bytes", C.c_int64)] + [(f, C.c_void_p) for f in ("seq_off", "seq", "qual", "flag", "pos", "end")]


class DbgWinsC(C.Structure):               # gbx_dbg_wins
    _fields_ = [("n_win", C.c_int64), ("ref_bytes", C.c_int64)] + [(f, C.c_void_p) for f in ("ref_off", "ref", "ref_pos", "read_lo", "read_hi")]


def make_params(k=15, min_qual=20, region_size=1500):
    return DbgParams(int(k), int(min_qual), int(region_size), 0)


class Refusal(ValueError):
    """A read the reference refuses (common.cpp getRead): its message, and the driver exits with status 1."""


class DbgReads:
    """Reads in file order: ASCII bases seq[seq_off[r] .. seq_off[r+1]), raw qualities, flags, the soft-clip-adjusted uint32
    pos and bam_endpos as uint32."""

    def __init__(self, seq_off, seq, qual, flag, pos, end, names=None):
        self.seq_off = np.ascontiguousarray(seq_off, dtype=np.int64)
        self.seq = np.ascontiguousarray(seq, dtype=np.uint8)
        self.qual = np.ascontiguousarray(qual, dtype=np.uint8)
        self.flag = np.ascontiguousarray(flag, dtype=np.uint16)
        self.pos = np.ascontiguousarray(pos, dtype=np.uint32)
        self.end = np.ascontiguousarray(end, dtype=np.uint32)
        self.names = names

    @property
    def n_reads(self):
        return int(self.flag.size)

    def read(self, r):
        a, b = int(self.seq_off[r]), int(self.seq_off[r + 1])
        return self.seq[a:b].tobytes(), self.qual[a:b].tobytes(), int(self.flag[r])

    def longest(self):
        if not self.n_reads:
            return 0
        return max(0, int((self.end - self.pos).astype(np.uint32).view(np.int32).max()))

    def c_struct(self):
        return DbgReadsC(self.n_reads, self.seq.size, *(N.ptr(a) for a in (self.seq_off, self.seq, self.qual, self.flag, self.pos, self.end)))

    @classmethod
    def from_list(cls, reads):
        """reads: [(seq bytes, qual bytes, flag, pos, end)]"""
        lens = [len(r[0]) for r in reads]
        off = np.zeros(len(reads) + 1, dtype=np.int64)
        off[1:] = np.cumsum(lens)
        cat = lambda xs: np.frombuffer(b"".join(xs), dtype=np.uint8)  # noqa: E731
        return cls(off, cat([r[0] for r in reads]), cat([r[1] for r in reads]), [r[2] for r in reads], [r[3] & 0xffffffff for r in reads],
                   [r[4] & 0xffffffff for r in reads])


def endpos(rec):
    """bam_endpos (UPSTREAM): pos + the reference length of the CIGAR, or pos + 1 when unmapped or of length 0."""
    rlen = 0 if rec["flag"] & 4 else P._ref_len(rec["cigar_words"])
    return rec["pos"] + (rlen if rlen > 0 else 1)


def check_record(rec):
    """The reference's refusals of a read, in its order (common.cpp:37-60); None when it is accepted."""
    if len(rec["name"].encode()) + 1 > MAX_READNAME_LEN:
        return "The maximum read name length is set to %d, but the actual read length is %d" % (MAX_READNAME_LEN, len(rec["name"].encode()) + 1)
    if rec["l_seq"] == 0:
        return "The sequence length is 0. How come?"
    if rec["qual"][0] == 0xFF:
        return "The quality score is 255 for the first base. How come?"
    if rec["l_seq"] + 1 > MAX_READ_LEN:
        return "The maximum read length is set to %d, but the actual read length is %d" % (MAX_READ_LEN, rec["l_seq"] + 1)
    if rec["cigar_words"].size > MAX_N_CIGAR:
        return "The maximum number of cigar is set to %d, but the actual number of cigar is %d" % (MAX_N_CIGAR, rec["cigar_words"].size)
    return None


def read_bam(path, region):
    """Every record of the region in file order (UPSTREAM, the region iterator: on the contig, pos < end and bam_endpos >
    beg) -> (DbgReads, (contig, beg, end), contig length).  A read the reference refuses raises Refusal."""
    contigs, recs = P.read_bam_file(path)
    lengths = dict(contigs)
    name, beg, end = P.parse_region(region, lengths)
    if name not in lengths:
        raise ValueError("contig '%s' is not in the BAM header" % name)
    tid = [c for c, _ in contigs].index(name)
    out = []
    for r in recs:
        if r["tid"] != tid or r["pos"] < 0 or r["pos"] >= end or endpos(r) <= beg:
            continue
        why = check_record(r)
        if why:
            raise Refusal(why)
        packed = r["packed"]
        codes = np.empty(2 * packed.size, dtype=np.uint8)
        codes[0::2], codes[1::2] = packed >> 4, packed & 15
        seq = _NT16[codes[:r["l_seq"]]].tobytes()
        cw = r["cigar_words"]
        pos = r["pos"]
        if cw.size and (int(cw[0]) & 15) == 4:
            pos -= int(cw[0]) >> 4
        out.append((seq, r["qual"].tobytes(), r["flag"], pos, endpos(r), r["name"]))
    rs = DbgReads.from_list([o[:5] for o in out])
    rs.names = [o[5] for o in out]
    return rs, (name, beg, end), lengths[name]


def read_fasta(path):
    """{name: bytes as stored} of a plain FASTA (the name is the header up to the first white space)."""
    out, name, parts = {}, None, []
    with open(path, "rb") as f:
        for line in f:
            line = line.rstrip(b"\r\n")
            if line.startswith(b">"):
                if name is not None:
                    out[name] = b"".join(parts)
                name, parts = line[1:].split()[0].decode() if line[1:].split() else "", []
            elif name is not None:
                parts.append(line)
    if name is not None:
        out[name] = b"".join(parts)
    return out


def fetch(contig_seq, start, end_incl):
    """faidx_fetch_seq(start, end_incl) (UPSTREAM): the bytes as stored, the end clamped to the contig."""
    end_incl = min(end_incl, len(contig_seq) - 1)
    return contig_seq[start:end_incl + 1] if start <= end_incl else b""


def window_ranges(reads, beg, end, params=None):
    """gbx_dbg_windows -> dict of int64 arrays (assem_start, assem_end, ref_start, ref_end, read_lo, read_hi); raises
    N.GbxError when the reference stops (lo > hi), with .window = (w, lo, hi)."""
    p = params or make_params()
    L = N.lib()
    rc_ = reads.c_struct()
    n = C.c_int64(0)
    rc = L.gbx_dbg_windows(C.byref(p), C.byref(rc_), int(beg), int(end), 0, C.byref(n), None, None, None, None, None, None)
    if rc not in (0, N.GBX_ERR_ARG):
        N.check(rc)
    cap = max(n.value, 1)
    arr = {f: np.zeros(cap, dtype=np.int64) for f in ("assem_start", "assem_end", "ref_start", "ref_end", "read_lo", "read_hi")}
    rc = L.gbx_dbg_windows(C.byref(p), C.byref(rc_), int(beg), int(end), cap, C.byref(n), *(N.ptr(arr[f]) for f in arr))
    if rc:
        e = N.GbxError(rc, L.gbx_last_error().decode())
        w = n.value - 1
        e.window = (w, int(arr["assem_start"][w]), int(arr["assem_end"][w]), int(arr["read_lo"][w]), int(arr["read_hi"][w])) if w >= 0 else None
        raise e
    return {f: a[:n.value] for f, a in arr.items()}


class DbgWins:
    """Windows with their reference bytes: ref[ref_off[w] .. ref_off[w+1]), ref_pos, reads [read_lo, read_hi)."""

    def __init__(self, ref_off, ref, ref_pos, read_lo, read_hi, assem_start=None, assem_end=None):
        self.ref_off = np.ascontiguousarray(ref_off, dtype=np.int64)
        self.ref = np.ascontiguousarray(ref, dtype=np.uint8)
        self.ref_pos = np.ascontiguousarray(ref_pos, dtype=np.int64)
        self.read_lo = np.ascontiguousarray(read_lo, dtype=np.int64)
        self.read_hi = np.ascontiguousarray(read_hi, dtype=np.int64)
        self.assem_start, self.assem_end = assem_start, assem_end

    @property
    def n_win(self):
        return int(self.ref_pos.size)

    def window_ref(self, w):
        return self.ref[self.ref_off[w]:self.ref_off[w + 1]].tobytes()

    def c_struct(self):
        return DbgWinsC(self.n_win, self.ref.size, *(N.ptr(a) for a in (self.ref_off, self.ref, self.ref_pos, self.read_lo, self.read_hi)))

    def occ_slots(self, reads, k):
        """per window: max(0, ref_len - k - 1) + the sum over its reads of max(0, l_seq - k - 1)"""
        rc = np.zeros(reads.n_reads + 1, dtype=np.int64)
        rc[1:] = np.cumsum(np.maximum(0, np.diff(reads.seq_off) - k - 1))
        return np.maximum(0, np.diff(self.ref_off) - k - 1) + rc[self.read_hi] - rc[self.read_lo]


def make_windows(reads, beg, end, contig_seq, params=None):
    wr = window_ranges(reads, beg, end, params)
    refs = [fetch(contig_seq, int(a), int(b) - 1) for a, b in zip(wr["ref_start"], wr["ref_end"])]
    off = np.zeros(len(refs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r) for r in refs])
    return DbgWins(off, np.frombuffer(b"".join(refs), dtype=np.uint8), wr["ref_start"], wr["read_lo"], wr["read_hi"], wr["assem_start"],
                   wr["assem_end"])


def build_host(reads, wins, params=None):
    """gbx_dbg_build_host -> STATS_DTYPE[n_win]"""
    p = params or make_params()
    st = np.zeros(max(wins.n_win, 1), dtype=STATS_DTYPE)
    r, w = reads.c_struct(), wins.c_struct()
    N.check(N.lib().gbx_dbg_build_host(C.byref(p), C.byref(r), C.byref(w), N.ptr(st)))
    return st[:wins.n_win]


def graph_host(reads, wins, stats, w0=0, w1=None, params=None):
    """gbx_dbg_graph_host for windows [w0, w1) -> (nodes NODE_DTYPE, edges EDGE_DTYPE, node_off, edge_off)"""
    p = params or make_params()
    w1 = wins.n_win if w1 is None else w1
    node_off = np.zeros(w1 - w0 + 1, dtype=np.int64)
    edge_off = np.zeros(w1 - w0 + 1, dtype=np.int64)
    node_off[1:] = np.cumsum(stats["n_nodes"][w0:w1])
    edge_off[1:] = np.cumsum(stats["n_edges"][w0:w1])
    nodes = np.zeros(max(int(node_off[-1]), 1), dtype=NODE_DTYPE)
    edges = np.zeros(max(int(edge_off[-1]), 1), dtype=EDGE_DTYPE)
    r, w = reads.c_struct(), wins.c_struct()
    N.check(N.lib().gbx_dbg_graph_host(C.byref(p), C.byref(r), C.byref(w), int(w0), int(w1), N.ptr(node_off), N.ptr(edge_off), N.ptr(nodes),
                                       N.ptr(edges)))
    return nodes[:node_off[-1]], edges[:edge_off[-1]], node_off, edge_off


def render(reads, wins, nodes, edges, node_off, edge_off, k, j):
    """Window j of a graph_* result as dbg_ref's node dicts (kmer from node_src, edges [end, weight])."""
    out = []
    for x in range(int(node_off[j]), int(node_off[j + 1])):
        nd = nodes[x]
        src = int(nd["src"])
        km = wins.ref[src:src + k].tobytes() if src >= 0 else reads.seq[-1 - src:-1 - src + k].tobytes()
        e0 = int(nd["first_edge"])
        out.append(dict(kmer=km, colours=int(nd["colours"]), position=int(nd["position"]), weight=int(nd["weight"]),
                        edges=[[int(edges[e]["end"]), int(edges[e]["weight"])] for e in range(e0, e0 + int(nd["n_edges"]))]))
    return out


def print_line(wins, w, st):
    """One line of `dbg --print`: assem_start assem_end ref_start read_lo read_hi, the stats, the digest in hex."""
    s = st[w] if not isinstance(st, dict) else st
    return "%d\t%d\t%d\t%d\t%d\t%s\t%016x" % (int(wins.assem_start[w]), int(wins.assem_end[w]), int(wins.ref_pos[w]), int(wins.read_lo[w]),
                                             int(wins.read_hi[w]), "\t".join(str(int(s[f])) for f in STATS_FIELDS[:-1]), int(s["digest"]))


class DeviceDbg:
    """Reads and windows on a device; build() = one gbx_dbg_build_device call on `stream`."""

    def __init__(self, reads, wins, device, params=None, work_bytes=None):
        import torch
        self.p = params or make_params()
        self.dev = torch.device(device)
        t = lambda a: torch.from_numpy(np.array(a) if a.size else np.zeros(1, dtype=a.dtype)).to(self.dev)  # noqa: E731
        self.arrays = [t(a) for a in (reads.seq_off, reads.seq, reads.qual, reads.flag.view(np.int16), wins.ref_off, wins.ref, wins.ref_pos,
                                      wins.read_lo, wins.read_hi)]
        a = [x.data_ptr() for x in self.arrays]
        self.reads = DbgReadsC(reads.n_reads, reads.seq.size, a[0], a[1], a[2], a[3], None, None)
        self.wins = DbgWinsC(wins.n_win, wins.ref.size, a[4], a[5], a[6], a[7], a[8])
        self.n_win = wins.n_win
        occ = wins.occ_slots(reads, self.p.k)
        self.work_bytes = N.lib().gbx_dbg_workspace_bytes(C.byref(self.p), wins.n_win, reads.n_reads, int(occ.max()) if occ.size else 0)
        if work_bytes is not None:           # a smaller workspace: more, smaller batches of windows (at least the largest window)
            self.work_bytes = int(work_bytes)
        self.work = torch.empty(max(self.work_bytes, 1), dtype=torch.uint8, device=self.dev)
        self.stats = torch.zeros(max(wins.n_win, 1) * STATS_DTYPE.itemsize, dtype=torch.uint8, device=self.dev)

    def build(self, stream=None):
        N.check(N.lib().gbx_dbg_build_device(C.byref(self.p), C.byref(self.reads), C.byref(self.wins), self.stats.data_ptr(), self.work.data_ptr(),
                                             self.work_bytes, stream))

    def results(self):
        return self.stats.cpu().numpy().view(STATS_DTYPE)[:self.n_win].copy()

    def graph(self, stats, w0, w1, stream=None):
        import torch
        node_off = np.zeros(w1 - w0 + 1, dtype=np.int64)
        edge_off = np.zeros(w1 - w0 + 1, dtype=np.int64)
        node_off[1:] = np.cumsum(stats["n_nodes"][w0:w1])
        edge_off[1:] = np.cumsum(stats["n_edges"][w0:w1])
        dno, deo = torch.from_numpy(node_off).to(self.dev), torch.from_numpy(edge_off).to(self.dev)
        dn = torch.zeros(max(int(node_off[-1]), 1) * NODE_DTYPE.itemsize, dtype=torch.uint8, device=self.dev)
        de = torch.zeros(max(int(edge_off[-1]), 1) * EDGE_DTYPE.itemsize, dtype=torch.uint8, device=self.dev)
        N.check(N.lib().gbx_dbg_graph_device(C.byref(self.p), C.byref(self.reads), C.byref(self.wins), int(w0), int(w1), dno.data_ptr(),
                                             deo.data_ptr(), dn.data_ptr(), de.data_ptr(), self.work.data_ptr(), self.work_bytes, stream))
        torch.cuda.synchronize(self.dev)
        return (dn.cpu().numpy().view(NODE_DTYPE)[:node_off[-1]].copy(), de.cpu().numpy().view(EDGE_DTYPE)[:edge_off[-1]].copy(), node_off,
                edge_off)
