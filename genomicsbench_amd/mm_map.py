"""minimap2 behind the chain scores (include/gbx.h): chains, regions, parents, selection, mapq and PAF text.

``DeviceMmMapper`` takes a ``DeviceMmSeeder`` and queues seed -> chain -> map -> PAF on one stream: reads in, what
``minimap2 -x map-ont`` prints without ``-c`` out.  All arithmetic in libgbx.so on the GPU.
"""
import ctypes as C

import numpy as np

from . import _native as N
from . import mm_stage as ST
from .mm_stage import LINE_ROOM, c as _c, pack_seqs as pack_names      # noqa: F401  (LINE_ROOM, pack_names: part of this module's interface)

REG_DTYPE = np.dtype([(k, "<i4") for k in ("id", "parent", "score", "subsc", "cnt", "as", "rid", "rev", "rs", "re", "qs", "qe", "mlen", "blen",
                                           "n_sub", "mapq")] + [("hash", "<u4"), ("read", "<i4")])
assert REG_DTYPE.itemsize == 72                              # sizeof(gbx_mm_reg)


class MmMapParams(C.Structure):
    _fields_ = [("min_cnt", C.c_int32), ("min_chain_score", C.c_int32), ("mask_level", C.c_float), ("pri_ratio", C.c_float),
                ("best_n", C.c_int32), ("min_diff", C.c_int32)]


@N.declare_once
def lib(L):
    """libgbx.so with the gbx_mm_map_* and gbx_mm_paf_* entries declared"""
    vp, i64, sz = C.c_void_p, C.c_int64, C.c_size_t
    P = C.POINTER(MmMapParams)
    L.gbx_mm_map_default_params.argtypes = [P]
    L.gbx_mm_map_default_params.restype = None
    L.gbx_mm_map_check_params.argtypes = [P]
    L.gbx_mm_map_workspace_bytes.argtypes = [i64, i64, i64]
    L.gbx_mm_map_workspace_bytes.restype = sz
    L.gbx_mm_map_device.argtypes = [P, i64, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, i64, vp, vp, sz, vp]
    L.gbx_mm_map_host.argtypes = [P, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, i64, vp]
    L.gbx_mm_paf_workspace_bytes.argtypes = [i64, i64]
    L.gbx_mm_paf_workspace_bytes.restype = sz
    L.gbx_mm_paf_device.argtypes = [i64, vp, vp, vp, i64, vp, vp, vp, vp, i64, vp, vp, vp, vp, i64, vp, vp, vp, sz, vp]
    L.gbx_mm_paf_host.argtypes = [i64, vp, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, i64, vp, C.POINTER(C.c_int64)]


def make_params(**kw):
    """gbx_mm_map_default_params with the given fields replaced (min_cnt, min_chain_score, mask_level, pri_ratio, best_n, min_diff)"""
    return N.fill_params(MmMapParams, lib().gbx_mm_map_default_params, kw, "gbx_mm_map_params")


def check_params(p):
    N.check(lib().gbx_mm_map_check_params(C.byref(p)))


def x31(name):
    h = name[0] if name else 0
    for c in name[1:]:
        h = ((h << 5) - h + c) & 0xffffffff
    return h


def wang(key):
    m = 0xffffffff
    key = (key + (~(key << 15) & m)) & m
    key ^= key >> 10
    key = (key + (key << 3)) & m
    key ^= key >> 6
    key = (key + (~(key << 11) & m)) & m
    key ^= key >> 16
    return key


def read_hash(name, qlen):
    """what minimap2 seeds a read's region hashes with: X31(name) ^ (W(qlen) + W(11))"""
    name = name.encode() if isinstance(name, str) else bytes(name)
    return x31(name) ^ ((wang(qlen & 0xffffffff) + wang(11)) & 0xffffffff)


def map_host(p, off, ax, ay, score, parent, peak, seq_off, rep_len, hashes, chain_cap=None, reg_cap=None):
    """gbx_mm_map_host -> dict(chain_off, u, cax, cay, n_chained, reg_off, regs, counts).  Capacities None: one per anchor (always enough)."""
    off, seq_off = _c(off, np.int64), _c(seq_off, np.int64)
    n, na = len(off) - 1, int(off[-1])
    chain_cap = max(na, 1) if chain_cap is None else chain_cap
    reg_cap = max(na, 1) if reg_cap is None else reg_cap
    ax, ay = _c(ax, np.uint64), _c(ay, np.uint64)
    f, q, v = _c(score, np.int32), _c(parent, np.int32), _c(peak, np.int32)
    rep, hs = _c(rep_len, np.int32), _c(hashes, np.uint32)
    chain_off, reg_off = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    u, regs = np.zeros(max(chain_cap, 1), np.uint64), np.zeros(max(reg_cap, 1), REG_DTYPE)
    cax, cay, nc = np.zeros(max(na, 1), np.uint64), np.zeros(max(na, 1), np.uint64), np.zeros(max(n, 1), np.int32)
    cnt = np.zeros(2, np.int64)
    N.check(lib().gbx_mm_map_host(C.byref(p), n, N.ptr(off), N.ptr(ax), N.ptr(ay), N.ptr(f), N.ptr(q), N.ptr(v), N.ptr(seq_off), N.ptr(rep), N.ptr(hs),
                                  N.ptr(chain_off), N.ptr(u), chain_cap, N.ptr(cax), N.ptr(cay), N.ptr(nc), N.ptr(reg_off), N.ptr(regs), reg_cap,
                                  N.ptr(cnt)))
    return dict(chain_off=chain_off, u=u[:cnt[0]], cax=cax[:na], cay=cay[:na], n_chained=nc[:n], reg_off=reg_off, regs=regs[:cnt[1]],
                counts=(int(cnt[0]), int(cnt[1])))


def map_cpu(p, off, ax, ay, score, parent, peak, seq_off, rep_len, hashes):
    """The same rules compiled for the host (mm_map_rules.h in libgbx_mm_cpu.so), one thread -> the dict map_host gives.  What the
    device is held against where no restatement is at hand (smoke(), scripts/time_mm_map.py)."""
    off, seq_off = _c(off, np.int64), _c(seq_off, np.int64)
    n, m = len(off) - 1, max(int(off[-1]), 1)
    ins = [_c(ax, np.uint64), _c(ay, np.uint64), _c(score, np.int32), _c(parent, np.int32), _c(peak, np.int32), seq_off, _c(rep_len, np.int32),
           _c(hashes, np.uint32)]
    chain_off, reg_off, cnt = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64), np.zeros(2, np.int64)
    u, cax, cay, nc, regs = np.zeros(m, np.uint64), np.zeros(m, np.uint64), np.zeros(m, np.uint64), np.zeros(max(n, 1), np.int32), np.zeros(m, REG_DTYPE)
    ST.twin().gbx_mm_map_cpu(C.byref(p), n, N.ptr(off), *[N.ptr(a) for a in ins], N.ptr(chain_off), N.ptr(u), N.ptr(cax), N.ptr(cay), N.ptr(nc),
                             N.ptr(reg_off), N.ptr(regs), N.ptr(cnt))
    return dict(chain_off=chain_off, u=u[:cnt[0]], cax=cax[:int(off[-1])], cay=cay[:int(off[-1])], n_chained=nc[:n], reg_off=reg_off, regs=regs[:cnt[1]],
                counts=(int(cnt[0]), int(cnt[1])))


def paf_host(regs, reg_off, qnames, seq_off, rep_len, tnames, tseq_off, text_cap=None):
    """gbx_mm_paf_host -> (text bytes, line_off)"""
    return ST.paf_text(lib().gbx_mm_paf_host, _c(regs, REG_DTYPE), reg_off, qnames, seq_off, rep_len, tnames, tseq_off, text_cap)


class DeviceMmMapper(ST.Fits):
    """Reads -> PAF on one stream.  seeder: a DeviceMmSeeder (its index names the targets); read_names / ref_names default to
    read<i> / ref<i>.  chain_cap / reg_cap / text_cap None: sized from the anchor count (a kept chain has min_cnt anchors of its
    own), which run() reads for gbx_chain_device anyway; counts() reports the need when a given capacity was too small.
    align: True or a gbx_mm_align_params (mm_align.make_params) - run() then queues seed -> chain -> map -> align -> PAF with
    CIGAR (`minimap2 -c`), results() also gives alns and cigar, and self.aligner is the DeviceMmAligner with its own counts()."""

    FIT = (("chains", 0, "chain_cap"), ("regions", 1, "reg_cap"), ("bytes of text", 2, "text_cap"))

    def __init__(self, seeder, p=None, read_names=None, ref_names=None, chain_cap=None, reg_cap=None, text_cap=None, align=None):
        import torch
        self.seeder, self.device = seeder, seeder.device
        self.p = make_params() if p is None else p
        check_params(self.p)
        sd, ix = seeder, seeder.index
        self.read_names = ["read%d" % i for i in range(sd.n_reads)] if read_names is None else list(read_names)
        self.ref_names = ["ref%d" % i for i in range(ix.n_seqs)] if ref_names is None else list(ref_names)
        assert len(self.read_names) == sd.n_reads and len(self.ref_names) == ix.n_seqs
        t = lambda a: torch.from_numpy(a).to(self.device)
        qn, qo = pack_names(self.read_names)
        tn, to = pack_names(self.ref_names)
        pad = ST.pad
        self.qnames, self.qname_off, self.tnames, self.tname_off = t(pad(qn)), t(qo), t(pad(tn)), t(to)
        qlen = np.diff(sd.seq_off.cpu().numpy())
        self.hash = t(pad(np.array([read_hash(nm, int(ln)) for nm, ln in zip(self.read_names, qlen)], np.uint32).view(np.int32)))
        self.name_room = ST.name_room(self.read_names, self.ref_names)
        self.caps = (chain_cap, reg_cap, text_cap)
        self.chain_off = torch.zeros(sd.n_reads + 1, dtype=torch.int64, device=self.device)
        self.reg_off = torch.zeros(sd.n_reads + 1, dtype=torch.int64, device=self.device)
        self.line_off = torch.zeros(sd.n_reads + 1, dtype=torch.int64, device=self.device)
        self.n_chained = torch.zeros(max(sd.n_reads, 1), dtype=torch.int32, device=self.device)
        self.cnt = torch.zeros(3, dtype=torch.int64, device=self.device)          # chains, regions, bytes of text
        self.cb = None
        self.sized_for = None
        self.aligner = None
        if align is not None and align is not False:
            from . import mm_align as MA
            self.aligner = MA.DeviceMmAligner(self, None if align is True else align, text_cap=text_cap)

    def _size(self, n_anchors):
        import torch
        if self.sized_for == n_anchors:
            return
        sd, L = self.seeder, lib()
        e = ST.allocator(self.device)
        cc, rc, tc = self.caps
        self.chain_cap = max(n_anchors // self.p.min_cnt, 1) if cc is None else int(cc)
        self.reg_cap = self.chain_cap if rc is None else int(rc)
        self.text_cap = ST.text_cap(self.reg_cap, self.name_room) if tc is None else int(tc)
        self.u = e(self.chain_cap, torch.int64)
        self.cax, self.cay = e(sd.anchor_cap, torch.int64), e(sd.anchor_cap, torch.int64)
        self.regs = e(self.reg_cap * REG_DTYPE.itemsize, torch.uint8)
        self.lines = e(self.text_cap, torch.uint8)
        self.work_bytes = L.gbx_mm_map_workspace_bytes(sd.n_reads, sd.anchor_cap, self.chain_cap)
        self.work = e(self.work_bytes, torch.uint8)
        self.paf_work_bytes = L.gbx_mm_paf_workspace_bytes(sd.n_reads, self.reg_cap)
        self.paf_work = e(self.paf_work_bytes, torch.uint8)
        self.sized_for = n_anchors

    def run_seed_chain(self, stream=None):
        """seeding and chain; reads the anchor count (gbx_chain_device takes it on the host)"""
        self.seeder.run(stream)
        self.cb = self.seeder.chain_batch()
        self.cb.run(stream)
        self._size(self.cb.n_anchors)

    def run_map(self, stream=None):
        sd, cb = self.seeder, self.cb
        N.check(lib().gbx_mm_map_device(C.byref(self.p), sd.n_reads, sd.off.data_ptr(), sd.ax.data_ptr(), sd.ay.data_ptr(), sd.anchor_cap,
                                        cb.score.data_ptr(), cb.parent.data_ptr(), cb.peak.data_ptr(), sd.seq_off.data_ptr(), sd.rep_len.data_ptr(),
                                        self.hash.data_ptr(), self.chain_off.data_ptr(), self.u.data_ptr(), self.chain_cap, self.cax.data_ptr(),
                                        self.cay.data_ptr(), self.n_chained.data_ptr(), self.reg_off.data_ptr(), self.regs.data_ptr(), self.reg_cap,
                                        self.cnt.data_ptr(), self.work.data_ptr(), self.work_bytes, stream))

    def run_paf(self, stream=None):
        sd, ix = self.seeder, self.seeder.index
        N.check(lib().gbx_mm_paf_device(sd.n_reads, self.regs.data_ptr(), self.reg_off.data_ptr(), self.cnt.data_ptr() + 8, self.reg_cap,
                                        self.qnames.data_ptr(), self.qname_off.data_ptr(), sd.seq_off.data_ptr(), sd.rep_len.data_ptr(), ix.n_seqs,
                                        self.tnames.data_ptr(), self.tname_off.data_ptr(), ix.off.data_ptr(), self.lines.data_ptr(), self.text_cap,
                                        self.line_off.data_ptr(), self.cnt.data_ptr() + 16, self.paf_work.data_ptr(), self.paf_work_bytes, stream))

    def run(self, stream=None):
        """seed -> chain -> map -> PAF, all queued on `stream`"""
        self.run_seed_chain(stream)
        self.run_map(stream)
        if self.aligner is not None:
            self.aligner.run(stream)
        else:
            self.run_paf(stream)

    def counts(self):
        """(chains, regions, bytes of text) of the last run(); regions -1 when the chains did not fit.  Synchronises."""
        return tuple(int(v) for v in self.cnt.cpu().numpy())

    def results(self):
        """dict of numpy arrays, cut to the counts"""
        c, r, _ = self._need_fit()
        a = self.cb.n_anchors
        u64 = lambda t, n: t[:n].cpu().numpy().view(np.uint64)
        out = dict(chain_off=self.chain_off.cpu().numpy(), u=u64(self.u, c), cax=u64(self.cax, a), cay=u64(self.cay, a),
                   n_chained=self.n_chained[:self.seeder.n_reads].cpu().numpy(), reg_off=self.reg_off.cpu().numpy(),
                   regs=self.regs[:r * REG_DTYPE.itemsize].cpu().numpy().view(REG_DTYPE), line_off=self.line_off.cpu().numpy())
        if self.aligner is not None:
            out.update(self.aligner.results())
        return out

    def paf(self):
        """the PAF text of the last run()"""
        if self.aligner is not None:
            self._need_fit()
            return self.aligner.paf()
        _, _, t = self._need_fit()
        return self.lines[:t].cpu().numpy().tobytes().decode()
