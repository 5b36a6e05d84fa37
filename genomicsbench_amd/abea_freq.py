"""Host mirror of abea's methylation frequency stage (f5c meth-freq: freq_main, R/benchmarks/abea/src/freq.c:253-430).

A record is one line of the call-methylation TSV; the table has one row per genomic site: group size, called sites, methylated
calls, the first-seen sequence.  Records expand to items (one, or one per CG with ``split_groups``), a stable radix sort by
(contig, start, end) and a segmented reduction make the table, and the text is written from it: all in libgbx.so on the GPU
(one device).  ``parse_tsv`` is the one host-only piece.
"""
import numpy as np

from . import _native as N
from .abea_meth import SITE_DTYPE

RECORD_DTYPE = np.dtype([("contig", "<i4"), ("start", "<i4"), ("end", "<i4"), ("n_cpg", "<i4"), ("llr", "<f8"), ("seq_off", "<i8"),
                         ("seq_len", "<i4"), ("pad_", "<i4")])                                       # gbx_abea_freq_record
FSITE_DTYPE = np.dtype([("contig", "<i4"), ("start", "<i4"), ("end", "<i4"), ("group_size", "<i4"), ("called_sites", "<i4"),
                        ("called_sites_methylated", "<i4"), ("seq_off", "<i8"), ("seq_len", "<i4"), ("pad_", "<i4")])   # gbx_abea_freq_site
assert RECORD_DTYPE.itemsize == 40 and FSITE_DTYPE.itemsize == 40
COUNT, REDUCE, FILL, NCOUNTS = 1, 2, 4, 8                # GBX_ABEA_FREQ_COUNT / _REDUCE / _FILL / _NCOUNTS
SUM_OVERFLOW, POS_OVERFLOW, KEY_BITS, ITEMS = 1, 2, 4, 8
CPGS, MOTIFS = 1, 2                                      # header kinds
SPLIT_GROUP = b"split-group"


def _declare(L):
    vp, i64, i32, f64 = N.C.c_void_p, N.C.c_int64, N.C.c_int, N.C.c_double
    L.gbx_abea_freq_work.argtypes, L.gbx_abea_freq_work.restype = [i64, i64], i64
    L.gbx_abea_freq_device.argtypes = [i32, i64, vp, vp, f64, i32, i32, i32, i64, vp, vp, vp, i64, vp, i64, vp, vp]
    L.gbx_abea_freq_host.argtypes = [i64, vp, vp, i64, f64, i32, i64, vp, vp, i64, vp, vp]
    L.gbx_abea_freq_records_work.argtypes, L.gbx_abea_freq_records_work.restype = [i64], i64
    L.gbx_abea_freq_records_device.argtypes = [i32, i64, vp, vp, i64, vp, vp, vp, vp, i32, i32, vp, vp, i64, vp, i64, vp, vp]
    L.gbx_abea_freq_records_host.argtypes = [i64, vp, vp, i64, vp, vp, vp, vp, i32, i32, i64, vp, vp, i64, vp, vp]
    L.gbx_abea_freq_merge_device.argtypes = [i32, i64, vp, vp, i64, vp, vp, i32, i32, vp, vp, i64, vp, i64, vp, vp]
    L.gbx_abea_freq_merge_host.argtypes = [i64, vp, vp, i64, i64, vp, vp, i64, i64, vp, vp, i64, vp, vp]
    L.gbx_abea_freq_tsv_work.argtypes, L.gbx_abea_freq_tsv_work.restype = [i64], i64
    L.gbx_abea_freq_tsv_device.argtypes = [i32, i64, vp, vp, i64, vp, vp, i32, i32, vp, vp, i64, vp, vp]
    L.gbx_abea_freq_tsv_host.argtypes = [i64, vp, vp, i64, i64, vp, i32, i32, i64, vp, vp]
    L.gbx_abea_freq_parse_host.argtypes = [vp, i64, i64, vp, i64, vp, i64, vp, vp, vp, vp]


_lib = N.declare_once(_declare)


def bits_for(v):
    """the key bits a largest value needs (1 .. 31)"""
    return min(31, max(1, int(v).bit_length()))


def make_records(contig, start, end, n_cpg, llr, seqs):
    """records and their arena from parallel lists; seqs: bytes objects"""
    n = len(seqs)
    rec = np.zeros(n, RECORD_DTYPE)
    rec["contig"], rec["start"], rec["end"], rec["n_cpg"], rec["llr"] = contig, start, end, n_cpg, llr
    lens = np.array([len(s) for s in seqs], np.int64)
    rec["seq_len"] = lens
    rec["seq_off"] = np.concatenate([[0], np.cumsum(lens)[:-1]]) if n else []
    return rec, np.frombuffer(b"".join(seqs), np.uint8).copy()


def site_sequences(sites, arena):
    """the sequence column of a table: a list of bytes"""
    a = np.ascontiguousarray(arena, np.uint8).tobytes()
    return [SPLIT_GROUP if s["seq_len"] < 0 else a[int(s["seq_off"]):int(s["seq_off"]) + int(s["seq_len"])] for s in sites]


def _two_sized(call, dtype):
    """the sizing convention of the host entries: once with no room, then with the need"""
    need_a, need_b = np.zeros(1, np.int64), np.zeros(1, np.int64)
    rcode = call(0, None, need_a, 0, None, need_b)
    if rcode != 0 and not (rcode == N.GBX_ERR_ARG and (need_a[0] > 0 or need_b[0] > 0)):
        N.check(rcode)
    ca, cb = int(need_a[0]), int(need_b[0])
    out, arena = np.zeros(max(ca, 1), dtype), np.zeros(max(cb, 1), np.uint8)
    if ca:
        N.check(call(ca, out, need_a, cb, arena, need_b))
    return out[:ca], arena[:cb]


def freq_host(records, arena, threshold=2.5, split_groups=False, site_cap=None, seq_cap=None):
    """gbx_abea_freq_host -> (sites FSITE_DTYPE[n], seq_arena uint8[]).  Capacities given: one call with exactly that room."""
    records, arena = np.ascontiguousarray(records, RECORD_DTYPE), np.ascontiguousarray(arena, np.uint8)
    call = lambda cap, sites, ns, bcap, seqs, nb: _lib().gbx_abea_freq_host(len(records), N.ptr(records), N.ptr(arena), arena.size, float(threshold),
                                                                            1 if split_groups else 0, cap, N.ptr(sites), N.ptr(ns), bcap, N.ptr(seqs), N.ptr(nb))
    if site_cap is None and seq_cap is None:
        return _two_sized(call, FSITE_DTYPE)
    ns, nb = np.zeros(1, np.int64), np.zeros(1, np.int64)
    sites, seqs = np.zeros(max(site_cap, 1), FSITE_DTYPE), np.zeros(max(seq_cap, 1), np.uint8)
    N.check(call(site_cap, sites, ns, seq_cap, seqs, nb))
    return sites[:int(ns[0])], seqs[:int(nb[0])]


def records_host(sites, scores, contig_of_read, ref_off, ref_len, ref_arena, clip_start=-1, clip_end=-1):
    """gbx_abea_freq_records_host: the arrays gbx_abea_call_methylation_host returns -> (records, arena)"""
    sites = np.ascontiguousarray(sites, SITE_DTYPE)
    scores = np.ascontiguousarray(np.asarray(scores, np.float32).reshape(-1))
    contig = np.ascontiguousarray(contig_of_read, np.int32)
    ref_off, ref_len, ref_arena = np.ascontiguousarray(ref_off, np.int64), np.ascontiguousarray(ref_len, np.int32), np.ascontiguousarray(ref_arena, np.uint8)
    assert scores.size == 2 * len(sites) and len(contig) == len(ref_len) == len(ref_off)
    call = lambda cap, rec, nr, bcap, seqs, nb: _lib().gbx_abea_freq_records_host(len(sites), N.ptr(sites), N.ptr(scores), len(contig), N.ptr(contig), N.ptr(ref_off),
                                                                                  N.ptr(ref_len), N.ptr(ref_arena), clip_start, clip_end, cap, N.ptr(rec), N.ptr(nr),
                                                                                  bcap, N.ptr(seqs), N.ptr(nb))
    return _two_sized(call, RECORD_DTYPE)


def merge_host(sites_a, arena_a, sites_b, arena_b):
    """gbx_abea_freq_merge_host: the table of the concatenated input, A's records first"""
    sa, sb = np.ascontiguousarray(sites_a, FSITE_DTYPE), np.ascontiguousarray(sites_b, FSITE_DTYPE)
    aa, ab = np.ascontiguousarray(arena_a, np.uint8), np.ascontiguousarray(arena_b, np.uint8)
    call = lambda cap, sites, ns, bcap, seqs, nb: _lib().gbx_abea_freq_merge_host(len(sa), N.ptr(sa), N.ptr(aa), aa.size, len(sb), N.ptr(sb), N.ptr(ab), ab.size, cap,
                                                                                  N.ptr(sites), N.ptr(ns), bcap, N.ptr(seqs), N.ptr(nb))
    return _two_sized(call, FSITE_DTYPE)


def _names(contig_names):
    return [s.encode() if isinstance(s, str) else bytes(s) for s in contig_names]


def tsv_host(sites, arena, contig_names, header_kind=CPGS, with_header=True, cap=None):
    """gbx_abea_freq_tsv_host -> bytes: the text meth-freq prints for the table"""
    sites, arena = np.ascontiguousarray(sites, FSITE_DTYPE), np.ascontiguousarray(arena, np.uint8)
    names = _names(contig_names)
    arr = (N.C.c_char_p * max(len(names), 1))(*names)
    need = np.zeros(1, np.int64)

    def call(room):
        out = np.zeros(max(room, 1), np.uint8)
        return _lib().gbx_abea_freq_tsv_host(len(sites), N.ptr(sites), N.ptr(arena), arena.size, len(names), arr, header_kind, 1 if with_header else 0, room,
                                             N.ptr(out) if room else None, N.ptr(need)), out
    out = N.call_with_room(call, 0 if cap is None else int(cap), need, fixed=cap is not None)
    return out[:int(need[0])].tobytes()


def parse_tsv(text):
    """gbx_abea_freq_parse_host -> (records, arena, contig names (bytes, in strcmp order), header kind).  Where the reference exits,
    GbxError carries its message and ``bad_line`` its line number."""
    text = bytes(text)
    buf = np.frombuffer(text, np.uint8) if text else np.zeros(0, np.uint8)
    counts, kind, bad = np.zeros(4, np.int64), np.zeros(1, np.int32), np.zeros(1, np.int64)

    def call(rec, arena, names):
        return _lib().gbx_abea_freq_parse_host(N.ptr(buf) if len(buf) else None, len(buf), 0 if rec is None else len(rec), N.ptr(rec),
                                               0 if arena is None else len(arena), N.ptr(arena), 0 if names is None else len(names), N.ptr(names), N.ptr(counts),
                                               N.ptr(kind), N.ptr(bad))
    rcode = call(None, None, None)
    if rcode != 0 and bad[0] >= 0:
        err = N.GbxError(rcode, N.lib().gbx_last_error().decode())
        err.bad_line, err.message = int(bad[0]), N.lib().gbx_last_error().decode()
        raise err
    rec, arena, names = np.zeros(max(int(counts[0]), 1), RECORD_DTYPE), np.zeros(max(int(counts[1]), 1), np.uint8), np.zeros(max(int(counts[3]), 1), np.uint8)
    if rcode != 0:
        N.check(call(rec, arena, names))
    nm = names[:int(counts[3])].tobytes().split(b"\0")[:int(counts[2])]
    return rec[:int(counts[0])], arena[:int(counts[1])], nm, int(kind[0])


class DeviceAbeaFreq:
    """The stage resident in HBM (torch tensors).  Batches come in with add_records() (host arrays), add_sites() (the sites and
    scores of a call-methylation batch: the records are made on the device) or as the merge() of two filled tables.
    count(): the item offsets; size(): synchronises for the item count, allocates the workspace, runs sort and reduce,
    synchronises for the table's sizes and the flags (raises what the host entry would) and allocates the table; fill(): the
    table; results(): it on the host; text(): the TSV, written on the device.  Every tensor a launch reads or writes is held by the
    object (a stage's workspace until the next call of that stage), so the methods may be given any stream; where a method reads a count back it waits for that stream."""

    def __init__(self, device, threshold=2.5, split_groups=False, pos_bits=31, contig_bits=16):
        import torch
        self.torch, self.device = torch, device
        self.threshold, self.split, self.pos_bits, self.contig_bits = float(threshold), 1 if split_groups else 0, int(pos_bits), int(contig_bits)
        self.rec, self.arena = [], []                        # device batches: uint8 tensors
        self.n_records = self.n_items = self.n_sites = self.n_bytes = 0
        self.site_cap = self.seq_cap = 0
        self.counts = torch.zeros(NCOUNTS, dtype=torch.int64, device=device)
        self.sites = self.seq_arena = self.work = self.item_off = self.d_rec = self.d_arena = None
        self.merged = None
        self.held = []                                       # inputs and workspaces of launches queued on a caller's stream: they live as long as this object

    def _sync(self, stream):
        """before a read on the host: a stream other than torch's current one is waited for by name"""
        if stream:
            N.check(N.lib().gbx_stream_synchronize(stream))

    def _ready(self, stream):
        """before a launch on another stream: what torch queued on its own (zero fills, copies, the gather) is done"""
        if stream:
            self.torch.cuda.current_stream().synchronize()

    def _t(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    def _z(self, n, dt=None):
        return self.torch.zeros(max(int(n), 1), dtype=dt or self.torch.uint8, device=self.device)

    def add_records(self, records, arena):
        records, arena = np.ascontiguousarray(records, RECORD_DTYPE), np.ascontiguousarray(arena, np.uint8)
        self.rec.append(self._t(records.view(np.uint8).reshape(-1)) if len(records) else self._z(0)[:0])
        self.arena.append(self._t(arena) if arena.size else self._z(0)[:0])

    def add_sites(self, sites, scores, contig_of_read, ref_off, ref_len, ref_arena, clip_start=-1, clip_end=-1, stream=None):
        """sites: SITE_DTYPE, scores: float32[2 n] (host arrays or device tensors of their bytes); synchronises once, for the two sizes"""
        torch = self.torch
        dev = lambda a, dt: a if isinstance(a, torch.Tensor) else self._t(np.ascontiguousarray(a, dt))
        d_sites = sites if isinstance(sites, torch.Tensor) else self._t(np.ascontiguousarray(sites, SITE_DTYPE).view(np.uint8).reshape(-1))
        n = d_sites.numel() // SITE_DTYPE.itemsize
        d_scores = dev(scores, np.float32)
        contig, roff, rlen = dev(contig_of_read, np.int32), dev(ref_off, np.int64), dev(ref_len, np.int32)
        ref = ref_arena if isinstance(ref_arena, torch.Tensor) else self._t(np.concatenate([np.ascontiguousarray(ref_arena, np.uint8), np.zeros(16, np.uint8)]))
        work, off = self._z(_lib().gbx_abea_freq_records_work(n)), self._z(2 * (n + 1), torch.int64)
        p = lambda a: a.data_ptr() if a is not None else None
        rec = arena = None

        def run(pass_, rcap, bcap):
            self._ready(stream)
            N.check(_lib().gbx_abea_freq_records_device(pass_, n, p(d_sites), p(d_scores), contig.numel(), p(contig), p(roff), p(rlen), p(ref), clip_start, clip_end,
                                                        p(work), p(off), rcap, p(rec), bcap, p(arena), stream))
        run(COUNT, 0, 0)
        self._sync(stream)
        nr, nb = int(off[n].item()), int(off[2 * n + 1].item())
        rec, arena = self._z(nr * RECORD_DTYPE.itemsize), self._z(nb)
        run(FILL, nr, nb)
        self.held.append((d_sites, d_scores, contig, roff, rlen, ref, work, off))
        self.rec.append(rec[:nr * RECORD_DTYPE.itemsize])
        self.arena.append(arena[:nb])

    def _gather(self):
        """the batches as one record array and one arena (sequence offsets moved behind the earlier arenas)"""
        torch = self.torch
        base, parts = 0, []
        for r, a in zip(self.rec, self.arena):
            if r.numel():
                v = r.clone().view(torch.int64).view(-1, 5)
                v[:, 3] += base
                parts.append(v.view(-1))
            base += a.numel()
        self.d_rec = torch.cat(parts) if parts else self._z(5, torch.int64)
        self.n_records = sum(r.numel() for r in self.rec) // RECORD_DTYPE.itemsize
        self.d_arena = torch.cat(list(self.arena) + [self._z(16)])

    def _run(self, pass_, stream):
        p = lambda a: a.data_ptr() if a is not None else None
        self._ready(stream)
        N.check(_lib().gbx_abea_freq_device(pass_, self.n_records, p(self.d_rec), p(self.d_arena), self.threshold, self.split, self.pos_bits, self.contig_bits,
                                            self.n_items, p(self.work), p(self.item_off), p(self.counts), self.site_cap, p(self.sites), self.seq_cap,
                                            p(self.seq_arena), stream))

    def count(self, stream=None):
        self._sync(stream)                                   # add_sites may have filled a batch on it; the gather runs on torch's stream
        self._gather()
        self.n_items = 0
        self.item_off = self._z(self.n_records + 1, self.torch.int64)
        self.work = self._z(_lib().gbx_abea_freq_work(self.n_records, 0))
        self._run(COUNT, stream)

    def _take_counts(self, who, stream=None):
        self._sync(stream)
        c = self.counts.cpu().numpy()                        # synchronises
        self.flags = int(c[4])
        if self.flags & SUM_OVERFLOW:
            raise N.GbxError(N.GBX_ERR_UNSUPPORTED, "%s: a site's called_sites is above INT32_MAX" % who)
        if self.flags & POS_OVERFLOW:
            raise N.GbxError(N.GBX_ERR_UNSUPPORTED, "%s: a split position is above INT32_MAX" % who)
        if self.flags:
            raise N.GbxError(N.GBX_ERR_ARG, "%s: the device flagged its input (flags %d)" % (who, self.flags))
        self.n_sites, self.n_bytes = int(c[2]), int(c[3])

    def _alloc_table(self, site_cap, seq_cap):
        self.site_cap = self.n_sites if site_cap is None else int(site_cap)
        self.seq_cap = self.n_bytes if seq_cap is None else int(seq_cap)
        self.sites, self.seq_arena = self._z(self.site_cap * FSITE_DTYPE.itemsize), self._z(self.seq_cap)

    def size(self, site_cap=None, seq_cap=None, stream=None):
        self._sync(stream)
        self.n_items = int(self.counts[0].item())            # synchronises
        self.held.append(self.work)                          # the count pass's
        self.work = self._z(_lib().gbx_abea_freq_work(self.n_records, self.n_items))
        self._run(REDUCE, stream)
        self._take_counts("gbx_abea_freq_device", stream)
        self._alloc_table(site_cap, seq_cap)

    def fill(self, stream=None):
        if self.merged is not None:
            self._merge(FILL, stream)
        else:
            self._run(FILL, stream)

    def _merge(self, pass_, stream):
        a, b = self.merged
        p = lambda t: t.data_ptr() if t is not None else None
        self._ready(stream)
        N.check(_lib().gbx_abea_freq_merge_device(pass_, a.n_sites, p(a.sites), p(a.seq_arena), b.n_sites, p(b.sites), p(b.seq_arena), self.pos_bits,
                                                  self.contig_bits, p(self.work), p(self.counts), self.site_cap, p(self.sites), self.seq_cap, p(self.seq_arena),
                                                  stream))

    def merge(self, other, site_cap=None, seq_cap=None, stream=None):
        """-> a new, filled DeviceAbeaFreq: the table of this one's input followed by `other`'s"""
        m = DeviceAbeaFreq(self.device, self.threshold, self.split, max(self.pos_bits, other.pos_bits), max(self.contig_bits, other.contig_bits))
        m.merged = (self, other)
        n = self.n_sites + other.n_sites
        m.work = m._z(_lib().gbx_abea_freq_work(n, n))
        m._merge(REDUCE, stream)
        m._take_counts("gbx_abea_freq_merge_device", stream)
        m._alloc_table(site_cap, seq_cap)
        m._merge(FILL, stream)
        return m

    def results(self, stream=None):
        """(sites, seq_arena) on the host, as freq_host returns them; stream: the one fill() was given"""
        self._sync(stream)
        ns = min(self.n_sites, self.site_cap)
        return (self.sites[:ns * FSITE_DTYPE.itemsize].cpu().numpy().view(FSITE_DTYPE).copy(),
                self.seq_arena[:min(self.n_bytes, self.seq_cap)].cpu().numpy())

    def text(self, contig_names, header_kind=CPGS, with_header=True, cap=None, stream=None):
        """the TSV as bytes, written on the device; cap: the room (None: what it needs)"""
        torch = self.torch
        names = _names(contig_names)
        off = np.concatenate([[0], np.cumsum([len(s) for s in names])]).astype(np.int64)
        d_off, d_names = self._t(off), self._t(np.frombuffer(b"".join(names) + b"\0" * 16, np.uint8).copy())
        n = min(self.n_sites, self.site_cap)
        work, line_off = self._z(_lib().gbx_abea_freq_tsv_work(n)), self._z(n + 2, torch.int64)
        out = None
        p = lambda t: t.data_ptr() if t is not None else None

        def run(pass_, room):
            self._ready(stream)
            N.check(_lib().gbx_abea_freq_tsv_device(pass_, n, p(self.sites), p(self.seq_arena), len(names), p(d_off), p(d_names), header_kind,
                                                    1 if with_header else 0, p(work), p(line_off), room, p(out), stream))
        run(COUNT, 0)
        self._sync(stream)
        need = int(line_off[n + 1].item())
        room = need if cap is None else int(cap)
        self.text_need, self.line_off = need, line_off
        out = self.text_buf = self._z(room + 64)              # (64 bytes of slack behind the room)
        run(FILL, room)
        self.text_held = (d_off, d_names, work)              # until the next text()
        self._sync(stream)
        return out[:min(need, room)].cpu().numpy().tobytes()
