"""Host side of the pileup benchmark (R/benchmarks/pileup: medaka's calculate_pileup over a BAM region).

``write_bam`` writes a coordinate-sorted BAM (BGZF blocks, no index); ``read_bam`` is a pure-Python BGZF/BAM reader,
independent of the C++ one in csrc/drivers/bam_reader.h, that applies the benchmark's read filter (medaka_bamiter.c) and
keeps the reads of one contig that overlap a region.  ``parse_region`` is htslib's hts_parse_reg as the driver uses it.
``layout_host`` / ``count_host`` / ``DevicePileup`` call libgbx.so; all layout and counting happens there on the GPU.
"""
import ctypes as C
import struct
import zlib

import numpy as np

from . import _native as N

FEATLEN = 10
PLP_BASES = "acgtACGTdD"
BATCH_LEN = 100000                     # the driver's chunk_len (medaka_counts.c:525)
STATS_FIELDS = ("n_cols", "n_positions", "max_ins", "max_depth", "aligned_bases", "bad_read")
# BAM flags the read filter drops: UNMAP, SECONDARY, QCFAIL, DUP, SUPPLEMENTARY
FILTER_FLAGS = 0x4 | 0x100 | 0x200 | 0x400 | 0x800
CIGAR_OPS = "MIDNSHP=X"
NT16 = "=ACMGRSVTWYHKDBN"
_NT16_CODE = np.full(256, 15, dtype=np.uint8)
for _i, _c in enumerate(NT16):
    _NT16_CODE[ord(_c)] = _i
    _NT16_CODE[ord(_c.lower())] = _i
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


class PileupParams(C.Structure):        # gbx_pileup_params
    _fields_ = [("num_dtypes", C.c_int32), ("num_homop", C.c_int32), ("start", C.c_int64), ("end", C.c_int64),
                ("slice_positions", C.c_int64), ("weibull", C.c_int32), ("pad_", C.c_int32)]


class PileupReadsC(C.Structure):        # gbx_pileup_reads
    _fields_ = [("n_reads", C.c_int64), ("seq_bytes", C.c_int64)] + [(f, C.c_void_p) for f in
                ("pos", "cigar_off", "cigar", "seq_off", "seq_boff", "seq", "qual", "rev", "dtype")]


class LayoutStats(C.Structure):         # gbx_pileup_layout_stats
    _fields_ = [(f, C.c_int64) for f in STATS_FIELDS]


def n_features(num_dtypes, num_homop):
    return FEATLEN * int(num_dtypes) * int(num_homop)


class PileupReads:
    """Reads in BAM's encodings, sorted by pos: CIGAR words len << 4 | op, nt16 bases two a byte (high nibble first) from
    seq[seq_boff[r]], qualities qual[seq_off[r] .. seq_off[r+1]) (0xFF missing), rev 0/1, dtype index or -1."""

    def __init__(self, pos, cigar_off, cigar, seq_off, seq_boff, seq, qual, rev, dtype, names=None):
        self.pos = np.ascontiguousarray(pos, dtype=np.int32)
        self.cigar_off = np.ascontiguousarray(cigar_off, dtype=np.int64)
        self.cigar = np.ascontiguousarray(cigar, dtype=np.uint32)
        self.seq_off = np.ascontiguousarray(seq_off, dtype=np.int64)
        self.seq_boff = np.ascontiguousarray(seq_boff, dtype=np.int64)
        self.seq = np.ascontiguousarray(seq, dtype=np.uint8)
        self.qual = np.ascontiguousarray(qual, dtype=np.uint8)
        self.rev = np.ascontiguousarray(rev, dtype=np.uint8)
        self.dtype = np.ascontiguousarray(dtype, dtype=np.int8)
        self.names = names

    @property
    def n_reads(self):
        return int(self.pos.size)

    @property
    def n_bases(self):
        return int(self.seq_off[-1] - self.seq_off[0]) if self.pos.size else 0

    def read(self, r):
        """(pos, [(op, len)], nt16 codes uint8[l_seq], qual uint8[l_seq], rev, dtype) of read r."""
        c = self.cigar[self.cigar_off[r]:self.cigar_off[r + 1]]
        n = int(self.seq_off[r + 1] - self.seq_off[r])
        packed = self.seq[self.seq_boff[r]:self.seq_boff[r] + (n + 1) // 2]
        codes = np.empty(2 * packed.size, dtype=np.uint8)
        codes[0::2], codes[1::2] = packed >> 4, packed & 15
        return (int(self.pos[r]), [(int(w) & 15, int(w) >> 4) for w in c], codes[:n],
                self.qual[self.seq_off[r]:self.seq_off[r + 1]], int(self.rev[r]), int(self.dtype[r]))

    def checksum(self):
        """CRC-32 over every read's pos (int32), rev, dtype (one byte each), op count (uint32), CIGAR words, l_seq (int32),
        packed bases and qualities, in order: what `pileup --parse-only` prints."""
        crc = 0
        for r in range(self.n_reads):
            c0, c1 = int(self.cigar_off[r]), int(self.cigar_off[r + 1])
            n = int(self.seq_off[r + 1] - self.seq_off[r])
            b0 = int(self.seq_boff[r])
            crc = zlib.crc32(struct.pack("<iBbI", int(self.pos[r]), int(self.rev[r]), int(self.dtype[r]), c1 - c0), crc)
            crc = zlib.crc32(self.cigar[c0:c1].tobytes(), crc)
            crc = zlib.crc32(struct.pack("<i", n), crc)
            crc = zlib.crc32(self.seq[b0:b0 + (n + 1) // 2].tobytes(), crc)
            crc = zlib.crc32(self.qual[self.seq_off[r]:self.seq_off[r + 1]].tobytes(), crc)
        return "%08x" % crc

    def c_struct(self):
        """A gbx_pileup_reads over these host arrays (keep self alive while it is used)."""
        return PileupReadsC(self.n_reads, self.seq.size, *(N.ptr(a) for a in (
            self.pos, self.cigar_off, self.cigar, self.seq_off, self.seq_boff, self.seq, self.qual, self.rev, self.dtype)))

    @classmethod
    def from_records(cls, recs):
        """recs: dicts with pos, cigar [(op, len)], seq (nt16 codes), qual, rev, dtype (and optional name), sorted by pos."""
        n = len(recs)
        cig = [np.array([(ln << 4) | op for op, ln in r["cigar"]], dtype=np.uint32) for r in recs]
        lens = np.array([len(r["seq"]) for r in recs], dtype=np.int64)
        packed = [pack_nt16(np.asarray(r["seq"], dtype=np.uint8)) for r in recs]
        cigar_off = np.zeros(n + 1, dtype=np.int64)
        cigar_off[1:] = np.cumsum([c.size for c in cig])
        seq_off = np.zeros(n + 1, dtype=np.int64)
        seq_off[1:] = np.cumsum(lens)
        seq_boff = np.zeros(n, dtype=np.int64)
        if n > 1:
            seq_boff[1:] = np.cumsum([p.size for p in packed])[:-1]
        cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dtype=dt)  # noqa: E731
        return cls([r["pos"] for r in recs], cigar_off, cat(cig, np.uint32), seq_off, seq_boff, cat(packed, np.uint8),
                   cat([np.asarray(r["qual"], dtype=np.uint8) for r in recs], np.uint8), [r["rev"] for r in recs],
                   [r.get("dtype", 0) for r in recs], [r.get("name", "r%d" % i) for i, r in enumerate(recs)])


def pack_nt16(codes):
    codes = np.asarray(codes, dtype=np.uint8)
    pad = np.zeros(codes.size + (codes.size & 1), dtype=np.uint8)
    pad[:codes.size] = codes
    return ((pad[0::2] << 4) | pad[1::2]).astype(np.uint8)


def nt16_of_text(text):
    return _NT16_CODE[np.frombuffer(text.encode() if isinstance(text, str) else text, dtype=np.uint8)]


# ---------------------------------------------------------------------------------------------------------- region
def _parse_int(s):
    """hts_parse_decimal: digits with ',' separators, stops at the first other character."""
    v, seen = 0, False
    for ch in s:
        if ch == ",":
            continue
        if not ch.isdigit():
            break
        v, seen = v * 10 + ord(ch) - 48, True
    return v, seen


def parse_region(reg, contig_lengths=None):
    """hts_parse_reg as the driver uses it -> (contig, beg, end), 0-based half-open: 'chr' is the whole contig (end =
    its length, or 2^31 - 1 when unknown), 'chr:beg' runs to the end, 'chr:beg-end' takes beg 1-based (0 stays 0, as
    htslib clamps) and end inclusive.  Thousands separators are allowed.  Raises ValueError on a malformed region."""
    big = (1 << 31) - 1
    colon = reg.rfind(":")
    if colon < 0 or (contig_lengths is not None and reg in contig_lengths):
        name = reg
        return name, 0, (contig_lengths.get(name, big) if contig_lengths else big)
    name, rest = reg[:colon], reg[colon + 1:]
    if not name:
        raise ValueError("Failed to parse region: '%s'" % reg)
    end_known = contig_lengths.get(name, big) if contig_lengths else big
    if "-" in rest:
        a, b = rest.split("-", 1)
        beg, ok_a = _parse_int(a)
        end, ok_b = _parse_int(b)
        if not ok_a and a:
            raise ValueError("Failed to parse region: '%s'" % reg)
        if not ok_b:
            end = end_known
    else:
        beg, ok_a = _parse_int(rest)
        if not ok_a:
            raise ValueError("Failed to parse region: '%s'" % reg)
        end = end_known
    beg = max(beg - 1, 0)
    if end < beg:
        raise ValueError("Failed to parse region: '%s' (end before start)" % reg)
    return name, beg, end


def driver_batches(name, beg, end):
    """The driver's batches (medaka_counts.c:521-534): region strings 'name:i-min(i+100000,end)' for i = beg, beg + 100000
    ..., each parsed again by hts_parse_reg -> [(string, lo, hi)] with lo = max(i - 1, 0), hi = min(i + 100000, end)."""
    out = []
    i = beg
    while i < end:
        e = min(i + BATCH_LEN, end)
        out.append(("%s:%d-%d" % (name, i, e), max(i - 1, 0), e))
        i += BATCH_LEN
    return out


# ---------------------------------------------------------------------------------------------------------- BAM I/O
def _bgzf_block(data, level):
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    cdata = co.compress(data) + co.flush()
    bsize = 18 + len(cdata) + 8
    hdr = struct.pack("<4BI2BH2BHH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, 66, 67, 2, bsize - 1)
    return hdr + cdata + struct.pack("<II", zlib.crc32(data), len(data))


def bgzf_compress(data, level=1, threads=16):
    """BGZF blocks of at most 65 280 input bytes each, then the EOF marker."""
    chunks = [data[i:i + 65280] for i in range(0, len(data), 65280)]
    if len(chunks) > 64 and threads > 1:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(threads) as ex:
            blocks = list(ex.map(lambda c: _bgzf_block(c, level), chunks))
    else:
        blocks = [_bgzf_block(c, level) for c in chunks]
    return b"".join(blocks) + BGZF_EOF


def _reg2bin(beg, end):
    end -= 1
    if beg >> 14 == end >> 14:
        return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def bam_record(name, tid, pos, mapq, flag, cigar, seq, qual, tags=b""):
    """One BAM record: cigar [(op, len)], seq nt16 codes (uint8), qual uint8 (0xFF = missing), tags raw aux bytes."""
    nm = name.encode() + b"\0"
    cw = np.array([(ln << 4) | op for op, ln in cigar], dtype="<u4")
    rlen = sum(ln for op, ln in cigar if op in (0, 2, 3, 7, 8))
    seq = np.asarray(seq, dtype=np.uint8)
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(nm), mapq, _reg2bin(pos, pos + max(rlen, 1)), len(cigar), flag, seq.size, -1, -1, 0)
    rec = body + nm + cw.tobytes() + pack_nt16(seq).tobytes() + np.asarray(qual, dtype=np.uint8).tobytes() + tags
    return struct.pack("<i", len(rec)) + rec


def dt_tag(value):
    return b"DTZ" + value.encode() + b"\0"


def bam_header(contigs, text=b"@HD\tVN:1.6\tSO:coordinate\n"):
    out = [b"BAM\1", struct.pack("<i", len(text)), text, struct.pack("<i", len(contigs))]
    for name, ln in contigs:
        nm = name.encode() + b"\0"
        out += [struct.pack("<i", len(nm)), nm, struct.pack("<i", ln)]
    return b"".join(out)


def write_bam(path, contigs, records, level=1, threads=16):
    """contigs [(name, length)]; records: raw records (bam_record) in coordinate order."""
    data = bam_header(contigs) + b"".join(records)
    with open(path, "wb") as f:
        f.write(bgzf_compress(data, level, threads))


def bgzf_decompress(raw):
    """The inflated bytes of a BGZF file; ValueError on anything that is not BGZF or is cut short."""
    out, at = [], 0
    while at < len(raw):
        if len(raw) - at < 18:
            raise ValueError("truncated BGZF block header at byte %d" % at)
        id1, id2, cm, flg = raw[at], raw[at + 1], raw[at + 2], raw[at + 3]
        if id1 != 0x1f or id2 != 0x8b or cm != 8 or not (flg & 4):
            raise ValueError("not a BGZF file (bad block header at byte %d)" % at)
        xlen = struct.unpack_from("<H", raw, at + 10)[0]
        if at + 12 + xlen > len(raw):
            raise ValueError("truncated BGZF extra field at byte %d" % at)
        bsize, x = None, at + 12
        while x + 4 <= at + 12 + xlen:
            si1, si2, slen = raw[x], raw[x + 1], struct.unpack_from("<H", raw, x + 2)[0]
            if si1 == 66 and si2 == 67 and slen == 2 and x + 6 <= at + 12 + xlen:
                bsize = struct.unpack_from("<H", raw, x + 4)[0] + 1
            x += 4 + slen
        if bsize is None:
            raise ValueError("not a BGZF file (no BC field at byte %d)" % at)
        if bsize < 12 + xlen + 8 or at + bsize > len(raw):
            raise ValueError("truncated BGZF block at byte %d" % at)
        cdata = raw[at + 12 + xlen:at + bsize - 8]
        crc, isize = struct.unpack_from("<II", raw, at + bsize - 8)
        try:
            d = zlib.decompressobj(-15)
            data = d.decompress(cdata, 65536)
        except zlib.error as e:
            raise ValueError("corrupt BGZF block at byte %d: %s" % (at, e))
        if len(data) != isize or zlib.crc32(data) != crc:
            raise ValueError("corrupt BGZF block at byte %d (size or CRC)" % at)
        out.append(data)
        at += bsize
    return b"".join(out)


def read_bam_file(path):
    """-> (contigs [(name, length)], list of record dicts) of every record of a BAM file, in file order."""
    with open(path, "rb") as f:
        raw = f.read()
    data = bgzf_decompress(raw)
    if len(data) < 12 or data[:4] != b"BAM\1":
        raise ValueError("not a BAM file: %s" % path)
    def need(at, n):
        if at + n > len(data):
            raise ValueError("truncated BAM data at byte %d" % at)
    l_text = struct.unpack_from("<i", data, 4)[0]
    if l_text < 0:
        raise ValueError("bad BAM header")
    at = 8 + l_text
    need(at, 4)
    n_ref = struct.unpack_from("<i", data, at)[0]
    at += 4
    contigs = []
    for _ in range(max(n_ref, 0)):
        need(at, 4)
        ln = struct.unpack_from("<i", data, at)[0]
        if ln < 1:
            raise ValueError("bad BAM reference name")
        need(at, 4 + ln + 4)
        name = data[at + 4:at + 4 + ln - 1].decode()
        contigs.append((name, struct.unpack_from("<i", data, at + 4 + ln)[0]))
        at += 8 + ln
    recs = []
    while at < len(data):
        need(at, 4)
        bs = struct.unpack_from("<i", data, at)[0]
        if bs < 32:
            raise ValueError("bad BAM record size at byte %d" % at)
        need(at + 4, bs)
        tid, pos, l_rn, mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHi", data, at + 4)
        p = at + 36
        end = at + 4 + bs
        if l_seq < 0 or l_rn < 1 or p + l_rn + 4 * n_cig + (l_seq + 1) // 2 + l_seq > end:
            raise ValueError("bad BAM record at byte %d" % at)
        name = data[p:p + l_rn - 1].decode(errors="replace")
        p += l_rn
        cw = np.frombuffer(data, dtype="<u4", count=n_cig, offset=p)
        p += 4 * n_cig
        packed = np.frombuffer(data, dtype=np.uint8, count=(l_seq + 1) // 2, offset=p)
        p += (l_seq + 1) // 2
        qual = np.frombuffer(data, dtype=np.uint8, count=l_seq, offset=p)
        p += l_seq
        recs.append(dict(name=name, tid=tid, pos=pos, mapq=mapq, flag=flag, cigar_words=cw, packed=packed, l_seq=l_seq, qual=qual,
                         aux=data[p:end]))
        at = end
    return contigs, recs


def aux_z(aux, tag):
    """The value of a Z tag in raw aux bytes, or None (also for an aux block that cannot be walked)."""
    sizes = {ord("A"): 1, ord("c"): 1, ord("C"): 1, ord("s"): 2, ord("S"): 2, ord("i"): 4, ord("I"): 4, ord("f"): 4}
    t, p = tag.encode(), 0
    while p + 3 <= len(aux):
        key, typ = aux[p:p + 2], aux[p + 2]
        p += 3
        if typ in (ord("Z"), ord("H")):
            e = aux.find(b"\0", p)
            if e < 0:
                return None
            if key == t and typ == ord("Z"):
                return aux[p:e].decode(errors="replace")
            p = e + 1
        elif typ == ord("B"):
            if p + 5 > len(aux):
                return None
            sub, cnt = aux[p], struct.unpack_from("<i", aux, p + 1)[0]
            if cnt < 0:
                return None
            p += 5 + sizes.get(sub, 1) * cnt
        elif typ in sizes:
            p += sizes[typ]
        else:
            return None
    return None


def _ref_len(cw):
    ops, lens = cw & 15, cw >> 4
    return int(lens[np.isin(ops, (0, 2, 3, 7, 8))].sum())


def read_bam(path, region, dtypes=None):
    """The reads a pileup of `region` sees: the benchmark's filter (no UNMAP/SECONDARY/SUPPLEMENTARY/QCFAIL/DUP flag,
    mapq >= 1), on the region's contig, overlapping [beg, end) -> (PileupReads, (contig, beg, end)).  dtypes: the DT:Z
    values in order (None or one value: every read is dtype 0); a read without a matching value gets -1."""
    contigs, recs = read_bam_file(path)
    lengths = dict(contigs)
    name, beg, end = parse_region(region, lengths)
    if name not in lengths:
        raise ValueError("contig '%s' is not in the BAM header" % name)
    tid = [c for c, _ in contigs].index(name)
    keep = []
    for r in recs:
        if r["tid"] != tid or r["flag"] & FILTER_FLAGS or r["mapq"] < 1:
            continue
        rend = r["pos"] + _ref_len(r["cigar_words"])
        if rend <= beg or r["pos"] >= end:
            continue
        dt = 0
        if dtypes is not None and len(dtypes) > 1:
            v = aux_z(r["aux"], "DT")
            dt = dtypes.index(v) if v in dtypes else -1
        keep.append((r, dt))
    keep.sort(key=lambda x: x[0]["pos"])         # (stable: file order within a position)
    n = len(keep)
    cigar_off = np.zeros(n + 1, dtype=np.int64)
    seq_off = np.zeros(n + 1, dtype=np.int64)
    seq_boff = np.zeros(n, dtype=np.int64)
    for i, (r, _) in enumerate(keep):
        cigar_off[i + 1] = cigar_off[i] + r["cigar_words"].size
        seq_off[i + 1] = seq_off[i] + r["l_seq"]
        if i + 1 < n:
            seq_boff[i + 1] = seq_boff[i] + r["packed"].size
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dtype=dt)  # noqa: E731
    rs = PileupReads([r["pos"] for r, _ in keep], cigar_off, cat([r["cigar_words"] for r, _ in keep], np.uint32), seq_off, seq_boff,
                     cat([r["packed"] for r, _ in keep], np.uint8), cat([r["qual"] for r, _ in keep], np.uint8),
                     [(r["flag"] >> 4) & 1 for r, _ in keep], [d for _, d in keep], [r["name"] for r, _ in keep])
    return rs, (name, beg, end)


# ---------------------------------------------------------------------------------------------------------- entries
def make_params(start, end, num_dtypes=1, num_homop=5, slice_positions=0, weibull=0):
    return PileupParams(int(num_dtypes), int(num_homop), int(start), int(end), int(slice_positions), int(weibull), 0)


def _stats_dict(st):
    return {f: int(getattr(st, f)) for f in STATS_FIELDS}


def layout_host(reads, start, end, num_dtypes=1, num_homop=5, slice_positions=0):
    """gbx_pileup_layout_host -> (pos_col int64[end - start + 1], stats dict)."""
    p = make_params(start, end, num_dtypes, num_homop, slice_positions)
    pos_col = np.zeros(end - start + 1, dtype=np.int64)
    st = LayoutStats()
    cr = reads.c_struct()
    N.check(N.lib().gbx_pileup_layout_host(C.byref(p), C.byref(cr), N.ptr(pos_col), C.byref(st)))
    return pos_col, _stats_dict(st)


def count_host(reads, start, end, pos_col, p0=None, p1=None, num_dtypes=1, num_homop=5, slice_positions=0):
    """gbx_pileup_count_host over positions [p0, p1) -> (major int32[c], minor int32[c], counts uint32[c, F])."""
    p0 = start if p0 is None else p0
    p1 = end if p1 is None else p1
    p = make_params(start, end, num_dtypes, num_homop, slice_positions)
    F = n_features(num_dtypes, num_homop)
    c = int(pos_col[p1 - start] - pos_col[p0 - start])
    major = np.zeros(c, dtype=np.int32)
    minor = np.zeros(c, dtype=np.int32)
    counts = np.zeros((c, F), dtype=np.uint32)
    cr = reads.c_struct()
    N.check(N.lib().gbx_pileup_count_host(C.byref(p), C.byref(cr), N.ptr(np.ascontiguousarray(pos_col, dtype=np.int64)), int(p0), int(p1),
                                          N.ptr(major), N.ptr(minor), N.ptr(counts)))
    return major, minor, counts


def pileup_host(reads, start, end, num_dtypes=1, num_homop=5, slice_positions=0):
    """layout then count of the whole region -> (pos_col, stats, major, minor, counts)."""
    pos_col, st = layout_host(reads, start, end, num_dtypes, num_homop, slice_positions)
    return (pos_col, st) + count_host(reads, start, end, pos_col, num_dtypes=num_dtypes, num_homop=num_homop,
                                      slice_positions=slice_positions)


class DevicePileup:
    """Device-resident reads, layout and workspace; layout() and count() = one gbx_pileup_*_device call each on `stream`."""

    def __init__(self, reads, device, start, end, num_dtypes=1, num_homop=5):
        import torch
        self.dev = torch.device(device)
        t = lambda a: torch.from_numpy(a if a.size else np.zeros(1, dtype=a.dtype)).to(self.dev)  # noqa: E731
        self.arrays = [t(a) for a in (reads.pos, reads.cigar_off, reads.cigar.view(np.int32), reads.seq_off, reads.seq_boff, reads.seq,
                                      reads.qual, reads.rev, reads.dtype)]
        self.reads = PileupReadsC(reads.n_reads, reads.seq.size, *(a.data_ptr() for a in self.arrays))
        self.start, self.end = int(start), int(end)
        self.params = make_params(start, end, num_dtypes, num_homop)
        self.F = n_features(num_dtypes, num_homop)
        self.pos_col = torch.zeros(self.end - self.start + 1, dtype=torch.int64, device=self.dev)
        self.stats = torch.zeros(len(STATS_FIELDS), dtype=torch.int64, device=self.dev)
        wb = N.lib().gbx_pileup_workspace_bytes(C.byref(self.params), reads.n_reads, int(reads.cigar.size))
        self.work = torch.empty(max(wb, 1), dtype=torch.uint8, device=self.dev)
        self.work_bytes = wb

    def layout(self, stream=None):
        N.check(N.lib().gbx_pileup_layout_device(C.byref(self.params), C.byref(self.reads), self.pos_col.data_ptr(), self.stats.data_ptr(),
                                                 self.work.data_ptr(), self.work_bytes, stream))

    def layout_results(self):
        return self.pos_col.cpu().numpy().copy(), dict(zip(STATS_FIELDS, (int(v) for v in self.stats.cpu().tolist())))

    def alloc_counts(self, n_cols):
        import torch
        self.major = torch.zeros(max(n_cols, 1), dtype=torch.int32, device=self.dev)
        self.minor = torch.zeros(max(n_cols, 1), dtype=torch.int32, device=self.dev)
        self.counts = torch.zeros(max(n_cols, 1) * self.F, dtype=torch.int32, device=self.dev)

    def count(self, p0=None, p1=None, stream=None):
        p0 = self.start if p0 is None else int(p0)
        p1 = self.end if p1 is None else int(p1)
        N.check(N.lib().gbx_pileup_count_device(C.byref(self.params), C.byref(self.reads), self.pos_col.data_ptr(), p0, p1,
                                                self.major.data_ptr(), self.minor.data_ptr(), self.counts.data_ptr(), self.work.data_ptr(),
                                                self.work_bytes, stream))

    def count_results(self, n_cols):
        return (self.major[:n_cols].cpu().numpy().copy(), self.minor[:n_cols].cpu().numpy().copy(),
                self.counts[:n_cols * self.F].cpu().numpy().view(np.uint32).reshape(n_cols, self.F).copy())


# ---------------------------------------------------------------------------------------------------------- printing
def header_line(num_dtypes, num_homop, dtypes=None):
    """print_pileup_data's header (medaka_counts.c:189-203): with several dtypes only dtype x base names."""
    parts = ["pos\tins\t"]
    if num_dtypes > 1:
        for d in dtypes:
            parts += ["%s.%s\t" % (d, b) for b in PLP_BASES]
    else:
        for k in range(num_homop):
            parts += ["%s.%d\t" % (b, k + 1) for b in PLP_BASES]
    parts.append("depth\n")
    return "".join(parts)


def buffer_cols(pos_cols_per_position, lo, hi):
    """The reference's buffer_cols after a batch [lo, hi) (medaka_counts.c:350,365-375), from the batch's per-position
    column counts (0 where no read spans the position): start at 2 (hi - lo) and grow as calculate_pileup does."""
    buf = 2 * (hi - lo)
    n_cols = 0
    for i, c in enumerate(pos_cols_per_position):
        if c == 0:
            continue
        pos = lo + i
        max_ins = int(c) - 1
        n_cols += 1
        if n_cols + max_ins > buf and pos > lo:      # (at the batch's first position the reference divides by zero)
            cols_per_pos = np.float32(n_cols + max_ins) / np.float32(pos - lo)
            buf = max_ins + max(2 * buf, int(cols_per_pos) * (hi - lo))
        n_cols += max_ins
    return buf


def format_batch(major, minor, counts, num_dtypes, num_homop, dtypes, buf):
    """The --print text of one batch: print_pileup_data then the length line (medaka_counts.c:575-576)."""
    out = [header_line(num_dtypes, num_homop, dtypes)]
    for j in range(major.size):
        row = counts[j]
        out.append("%d\t%d\t%s\t%d\n" % (major[j], minor[j], "\t".join(str(int(v)) for v in row), int(row.sum())))
    out.append("pileup is length %d, with buffer of %d columns\n" % (major.size, buf))
    return "".join(out)
