"""SAM records: bwa-mem's mem_aln2sam, add_cigar and the MD part of bwa_gen_cigar2 on the GPU through gbx_mem_sam_* (include/gbx.h),
the stage behind the CIGAR stage.

Input: the regions of the regs stage (mode 0, single-end) or of the paired stage with its pair records (mode 1, 2 n_pairs
interleaved reads), what the CIGAR stage made of that stage's list, the reads with their names and qualities, and the contigs
with their names.  Output: one SAM_DTYPE record and one line of text per reported region, and one for a read with nothing
reported; the MD strings on their own as well.  ``DeviceMemSam`` stands behind a ``mem_cigar.DeviceMemCigar``; ``pipeline`` queues
regs -> pestat -> rescue -> pair -> cigar -> sam on one stream and returns the text.
"""
import ctypes as C

import numpy as np

from . import _native as N
from .mem_cigar import ALN_DTYPE
from .mem_pair import PAIR_DTYPE
from .mem_regs import REG_DTYPE

SAM_DTYPE = np.dtype([("pos", "<i8"), ("mpos", "<i8"), ("tlen", "<i8"), ("cigar_off", "<i8"), ("md_off", "<i8"), ("line_off", "<i8"),
                      ("read", "<i4"), ("which", "<i4"), ("flag", "<i4"), ("rid", "<i4"), ("mapq", "<i4"), ("mrid", "<i4"), ("nm", "<i4"),
                      ("as_", "<i4"), ("xs", "<i4"), ("n_cigar", "<i4"), ("md_len", "<i4"), ("sq_b", "<i4"), ("sq_e", "<i4"),
                      ("line_len", "<i4"), ("n_sa", "<i4"), ("pad_", "<i4")])
assert SAM_DTYPE.itemsize == 112


class SamParams(C.Structure):            # gbx_mem_sam_params
    _fields_ = [("softclip", C.c_int32), ("pad_", C.c_int32)]


@N.declare_once
def lib(L):
    """libgbx.so with the SAM entries declared (raises if the library or the entries are missing)."""
    vp, i64, i32, sz = C.c_void_p, C.c_int64, C.c_int32, C.c_size_t
    L.gbx_mem_sam_default_params.argtypes = [C.POINTER(SamParams)]
    L.gbx_mem_sam_default_params.restype = None
    L.gbx_mem_sam_workspace_bytes.argtypes = [i64, i64, i64]
    L.gbx_mem_sam_workspace_bytes.restype = sz
    L.gbx_mem_sam_text_cap.argtypes = [i64, i64, i64, i64, i32, i32, i32]
    L.gbx_mem_sam_text_cap.restype = sz
    L.gbx_mem_sam_device.argtypes = [C.POINTER(SamParams), i64, i32, vp, vp, vp, i64, vp, vp, i64, vp, vp, i64, vp, i64, vp, vp, vp,
                                     vp, vp, i64, vp, vp, i64, vp, i64, i64, i32, vp, vp, i64, vp, vp, vp, i64, vp, vp, i64, vp, vp, sz, vp]
    L.gbx_mem_sam_host.argtypes = [C.POINTER(SamParams), i64, i32, vp, vp, i64, vp, vp, i64, vp, i64, vp, i64, vp, vp, vp,
                                   vp, vp, i64, vp, vp, i64, vp, i64, i64, i32, vp, vp, i64, vp, C.POINTER(i64), vp, i64, C.POINTER(i64),
                                   vp, i64, C.POINTER(i64)]


def make_params(**kw):
    """bwa mem's default (softclip 0: supplementary records are hard-clipped) with the fields in `kw` replaced."""
    return N.fill_params(SamParams, lib().gbx_mem_sam_default_params, kw, "gbx_mem_sam_params")


def arena(items):
    """A list of byte strings (or str) -> (uint8 arena, int64 offsets[n + 1])."""
    items = [x.encode() if isinstance(x, str) else bytes(x) for x in items]
    off = np.zeros(len(items) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(x) for x in items])
    return np.frombuffer(b"".join(items), dtype=np.uint8).copy(), off


def text_cap(rec_cap, cigar_words, read_bytes, name_bytes, max_contig_name, max_recs=8, max_del=1024):
    """gbx_mem_sam_text_cap: a text_cap that suffices under the bounds given."""
    return int(lib().gbx_mem_sam_text_cap(int(rec_cap), int(cigar_words), int(read_bytes), int(name_bytes), int(max_contig_name),
                                          int(max_recs), int(max_del)))


def header(contig_names, contig_off, l_pac=None):
    """The @SQ lines of a SAM header: one per contig with its length.  l_pac, if given, must be the last offset."""
    co = np.asarray(contig_off, dtype=np.int64)
    assert len(co) == len(contig_names) + 1 and (l_pac is None or int(co[-1]) == int(l_pac))
    names = [x.decode() if isinstance(x, (bytes, bytearray)) else str(x) for x in contig_names]
    return "".join("@SQ\tSN:%s\tLN:%d\n" % (n, int(co[k + 1] - co[k])) for k, n in enumerate(names))


def sam_host(params, mode, regs, reg_off, pairs, alns, cigar, qer, read_off, read_len, qual, names, contig_names, text, l_pac, contig_off,
             rec_cap=None, md_cap=None, text_cap=None):
    """gbx_mem_sam_host -> dict(recs SAM_DTYPE[n_recs], rec_off, n_recs, md uint8[n_md], n_md, lines uint8[n_text], n_text).
    names / contig_names: lists of byte strings; qual: uint8 arena at the reads' offsets or None; pairs: PAIR_DTYPE records
    (mode 1) or None.  Without capacities the call is repeated once with the counts it reported."""
    regs = np.ascontiguousarray(regs).view(REG_DTYPE) if len(regs) else np.zeros(0, REG_DTYPE)
    reg_off = np.ascontiguousarray(reg_off, dtype=np.int64)
    alns = np.ascontiguousarray(alns, dtype=ALN_DTYPE)
    cigar = np.ascontiguousarray(cigar, dtype=np.uint32)
    qer = np.ascontiguousarray(qer, dtype=np.uint8)
    read_off = np.ascontiguousarray(read_off, dtype=np.int64)
    read_len = np.ascontiguousarray(read_len, dtype=np.int32)
    text = np.ascontiguousarray(text, dtype=np.uint8)
    contig_off = np.ascontiguousarray(contig_off, dtype=np.int64)
    qual = None if qual is None else np.ascontiguousarray(qual, dtype=np.uint8)
    pairs = None if pairs is None else np.ascontiguousarray(pairs, dtype=PAIR_DTYPE)
    nm, no = arena(names)
    cn, cno = arena(contig_names)
    n_reads = len(reg_off) - 1
    assert len(no) == n_reads + 1 and min(len(read_off), len(read_len)) >= n_reads and (qual is None or len(qual) == len(qer))
    sized = rec_cap is None and md_cap is None and text_cap is None
    rcap = n_reads + len(regs) if rec_cap is None else int(rec_cap)
    mcap = 0 if md_cap is None else int(md_cap)
    tcap = 0 if text_cap is None else int(text_cap)
    keep = np.zeros(2, np.int64)
    opt = lambda a: N.ptr(a) if a is not None and len(a) else None
    while True:
        recs = np.zeros(max(rcap, 1), dtype=SAM_DTYPE)
        rec_off = np.zeros(n_reads + 1, dtype=np.int64)
        md = np.zeros(max(mcap, 1), dtype=np.uint8)
        lines = np.zeros(max(tcap, 1), dtype=np.uint8)
        n_r, n_m, n_t = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        rc = lib().gbx_mem_sam_host(
            C.byref(params), n_reads, int(mode), opt(regs), N.ptr(reg_off), len(regs), opt(pairs), opt(alns), len(alns), opt(cigar), len(cigar),
            opt(qer), len(qer), N.ptr(read_off) if len(read_off) else N.ptr(keep), N.ptr(read_len) if len(read_len) else N.ptr(keep), opt(qual),
            opt(nm), N.ptr(no), len(nm), opt(cn), N.ptr(cno), len(cn), N.ptr(text), len(text), int(l_pac), len(contig_off) - 1,
            N.ptr(contig_off), N.ptr(recs), rcap, N.ptr(rec_off), C.byref(n_r), N.ptr(md), mcap, C.byref(n_m), N.ptr(lines), tcap, C.byref(n_t))
        if sized and rc == N.GBX_ERR_ARG and (n_m.value > mcap or n_t.value > tcap) and n_r.value <= rcap:
            mcap, tcap, sized = int(n_m.value), int(n_t.value), False
            continue
        N.check(rc)
        return dict(recs=recs[:n_r.value], rec_off=rec_off, n_recs=int(n_r.value), md=md[:n_m.value], n_md=int(n_m.value),
                    lines=lines[:n_t.value], n_text=int(n_t.value))


class DeviceMemSam:
    """gbx_mem_sam_device behind a ``mem_cigar.DeviceMemCigar`` that aligned the list of `stage`: a ``mem_pair.DeviceMemPair``
    (mode 1) or a ``mem_regs.DeviceMemRegs`` / ``mem_rescue.DeviceMemRescue`` (mode 0); the mode is whether the stage has
    ``pairs``, and its ``regions`` and ``batch`` records are what is read of it.  names: one byte string per read; qual: a
    uint8 array at the reads' offsets in the read arena, or None; contig_names: one byte string per contig.  run(stream) can be
    queued behind the CIGAR stage's run() on the same stream; no count is read on the host.  The capacities default to
    gbx_mem_sam_text_cap for reads with at most max_recs records and deletions of at most max_del bases."""

    def __init__(self, stage, cigar_stage, names, qual, contig_names, params=None, rec_cap=None, md_cap=None, text_cap=None, max_recs=8,
                 max_del=1024):
        import torch
        self.cigar_stage = cigar_stage
        b, rg = self.batch, self.regions = stage.batch, stage.regions
        self.pairs = stage.pairs
        self.mode = 0 if self.pairs is None else 1
        self.params = params or make_params()
        dev = self.device = b.device
        self.n_reads = b.n_reads
        nm, no = arena(names)
        cn, cno = arena(contig_names)
        assert len(no) == self.n_reads + 1 and len(cno) == b.n_contigs + 1
        t = lambda a: torch.from_numpy(a if len(a) else np.zeros(1, a.dtype)).to(dev)
        self.names, self.name_off, self.name_bytes = t(nm), t(no), len(nm)
        self.cnames, self.cname_off, self.cname_bytes = t(cn), t(cno), len(cn)
        self.qual = None
        if qual is not None:
            qual = np.ascontiguousarray(qual, dtype=np.uint8)
            assert len(qual) == b.qer_bytes
            self.qual = t(qual)
        self.rec_cap = int(self.n_reads + min(rg.cap, cigar_stage.n) if rec_cap is None else rec_cap)
        cap = lib().gbx_mem_sam_text_cap(self.rec_cap, cigar_stage.cigar_cap, b.qer_bytes, len(nm), int(np.diff(cno).max()), max_recs, max_del)
        self.text_cap = int(cap if text_cap is None else text_cap)
        self.md_cap = int(self.text_cap if md_cap is None else md_cap)
        self.recs = torch.zeros(max(self.rec_cap, 1) * SAM_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.rec_off = torch.zeros(self.n_reads + 1, dtype=torch.int64, device=dev)
        self.md = torch.zeros(max(self.md_cap, 1), dtype=torch.uint8, device=dev)
        self.lines = torch.zeros(max(self.text_cap, 1), dtype=torch.uint8, device=dev)
        self.counts = torch.zeros(3, dtype=torch.int64, device=dev)           # records, md bytes, text bytes
        self.work_bytes = lib().gbx_mem_sam_workspace_bytes(self.n_reads, rg.cap, cigar_stage.n)
        self.work = torch.empty(max(self.work_bytes, 1), dtype=torch.uint8, device=dev)

    def run(self, stream=None):
        """Asynchronous on `stream` (a raw hipStream_t handle or None)."""
        b, rg, cg = self.batch, self.regions, self.cigar_stage
        c = self.counts.data_ptr()
        N.check(lib().gbx_mem_sam_device(
            C.byref(self.params), self.n_reads, self.mode, rg.regs.data_ptr(), rg.reg_off.data_ptr(), rg.count.data_ptr(), rg.cap,
            self.pairs.data_ptr() if self.mode else None, cg.alns.data_ptr(), cg.n, cg.cigar.data_ptr(), cg.n_cigar.data_ptr(), cg.cigar_cap,
            b.qer.data_ptr(), b.qer_bytes, b.read_off.data_ptr(), b.read_len.data_ptr(), self.qual.data_ptr() if self.qual is not None else None,
            self.names.data_ptr(), self.name_off.data_ptr(), self.name_bytes, self.cnames.data_ptr(), self.cname_off.data_ptr(),
            self.cname_bytes, b.ref.data_ptr(), b.ref_bytes, b.l_pac, b.n_contigs, b.contig_off.data_ptr(), self.recs.data_ptr(),
            self.rec_cap, self.rec_off.data_ptr(), c, self.md.data_ptr(), self.md_cap, c + 8, self.lines.data_ptr(), self.text_cap, c + 16,
            self.work.data_ptr(), self.work_bytes, stream))

    def results(self):
        """dict(recs, rec_off, n_recs, md, n_md, lines, n_text) of the last run(); raises when a stage before it overflowed or a
        capacity was too small."""
        nr, nm, nt = (int(x) for x in self.counts.cpu().numpy())
        if nr < 0 or nm < 0 or nt < 0:
            raise RuntimeError("mem sam: a stage before it overflowed its capacities")
        if nr > self.rec_cap or nm > self.md_cap or nt > self.text_cap:
            raise RuntimeError("mem sam: %d records, %d md bytes and %d text bytes do not fit the capacities %d, %d and %d" %
                               (nr, nm, nt, self.rec_cap, self.md_cap, self.text_cap))
        return dict(recs=self.recs[:nr * SAM_DTYPE.itemsize].cpu().numpy().view(SAM_DTYPE).copy(), rec_off=self.rec_off.cpu().numpy(),
                    n_recs=nr, md=self.md[:nm].cpu().numpy(), n_md=nm, lines=self.lines[:nt].cpu().numpy(), n_text=nt)

    def text(self):
        """The SAM lines of the last run() as bytes."""
        return self.results()["lines"].tobytes()


def pipeline(ext, names, qual, contig_names, stream=None, pair_id0=0, sam_params=None, with_header=True, sam_caps=None, regs_params=None,
             rescue_params=None, pair_params=None, cigar_params=None, cigar_cap=None, z_bytes=None):
    """regs -> pestat -> rescue -> pair -> cigar -> sam on one stream behind a ``mem_chain.DeviceSeedExtension`` that has been
    queued on it (``mem_pipeline.Stages`` from "regs" on); the arguments are ``mem_rescue.pipeline``'s, and sam_caps goes to
    DeviceMemSam.  The stream is synchronised and the text read back.  -> (SAM text as bytes, (regs, rescue, pair, cigar, sam)
    stages)."""
    from .mem_pipeline import Stages
    caps = {k: v for k, v in dict(sam_caps or {}, cigar_cap=cigar_cap, z_bytes=z_bytes).items() if v is not None}
    st = Stages(ext=ext, id0=pair_id0, params=dict(regs=regs_params, rescue=rescue_params, pair=pair_params, cigar=cigar_params, sam=sam_params),
                caps=caps, sam_input=(names, qual, contig_names))
    st.queue(stream, "regs")
    N.check(N.lib().gbx_stream_synchronize(stream))
    b = ext.batch
    head = header(contig_names, b.contig_off.cpu().numpy(), b.l_pac).encode() if with_header else b""
    return head + st.sam.text(), (st.regs, st.rescue, st.pair, st.cigar, st.sam)
