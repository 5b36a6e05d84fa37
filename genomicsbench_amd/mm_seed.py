"""minimap2's seeding stage in front of chain (include/gbx.h): minimizer sketch, minimizer index, seed collection.

``DeviceMmIndex`` builds the index of a reference on the device; ``DeviceMmSeeder`` turns reads into the chain batch
(off, ax, ay, hdr) there, and ``chain_batch()`` hands those tensors to ``DeviceChainBatch.from_tensors``: reads -> anchors ->
chain scores on one stream.  All arithmetic in libgbx.so on the GPU.
"""
import ctypes as C

import numpy as np

from . import _native as N
from . import mm_stage as ST
from .mm_stage import pack_seqs                             # noqa: F401  (part of this module's interface)

SKETCH_CHUNK = 256                       # GBX_MM_SKETCH_CHUNK
SEED_TANDEM = 1 << 42
MAX_READS = 1 << 21


class MmParams(C.Structure):
    _fields_ = [("k", C.c_int32), ("w", C.c_int32), ("is_hpc", C.c_int32), ("mid_occ", C.c_int32), ("mid_occ_frac", C.c_float),
                ("max_gap", C.c_int32), ("bw", C.c_int32)]


class MmIndexInfo(C.Structure):
    _fields_ = [("n_keys", C.c_int64), ("n_vals", C.c_int64), ("mid_occ", C.c_int32), ("k", C.c_int32), ("w", C.c_int32),
                ("is_hpc", C.c_int32)]


@N.declare_once
def lib(L):
    """libgbx.so with the gbx_mm_* entries declared"""
    vp, i64, i32, sz = C.c_void_p, C.c_int64, C.c_int32, C.c_size_t
    P = C.POINTER(MmParams)
    L.gbx_mm_default_params.argtypes = [P]
    L.gbx_mm_default_params.restype = None
    L.gbx_mm_check_params.argtypes = [P]
    L.gbx_mm_sketch_workspace_bytes.argtypes = [P, i64, i64]
    L.gbx_mm_sketch_workspace_bytes.restype = sz
    L.gbx_mm_sketch_device.argtypes = [P, i64, vp, vp, i64, i32, vp, vp, i64, vp, vp, vp, sz, vp]
    L.gbx_mm_sketch_host.argtypes = [P, i64, vp, vp, i32, vp, vp, i64, vp, C.POINTER(C.c_int64)]
    L.gbx_mm_index_bytes.argtypes = [i64]
    L.gbx_mm_index_bytes.restype = sz
    L.gbx_mm_index_workspace_bytes.argtypes = [P, i64, i64, i64]
    L.gbx_mm_index_workspace_bytes.restype = sz
    L.gbx_mm_index_build_device.argtypes = [P, i64, vp, vp, i64, vp, i64, vp, sz, vp]
    L.gbx_mm_index_stats.argtypes = [vp, i64, C.POINTER(MmIndexInfo), vp]
    L.gbx_mm_index_build_host.argtypes = [P, i64, vp, vp, vp, vp, i64, vp, i64, C.POINTER(MmIndexInfo)]
    L.gbx_mm_seed_workspace_bytes.argtypes = [P, i64, i64, i64, i64]
    L.gbx_mm_seed_workspace_bytes.restype = sz
    L.gbx_mm_seed_device.argtypes = [P, vp, i64, i64, i64, i64, vp, vp, i64, vp, vp, i64, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, sz, vp]
    L.gbx_mm_seed_host.argtypes = [P, vp, vp, i64, vp, i32, i64, i64, i64, vp, vp, vp, vp, i64, vp, vp, vp, i64, vp, vp, vp, vp, vp]


def make_params(**kw):
    """gbx_mm_default_params with the given fields replaced (k, w, is_hpc, mid_occ, mid_occ_frac, max_gap, bw)"""
    return N.fill_params(MmParams, lib().gbx_mm_default_params, kw, "gbx_mm_params")


def check_params(p):
    N.check(lib().gbx_mm_check_params(C.byref(p)))


def sketch_host(p, seqs, rid_ordinal=True, mini_cap=None):
    """gbx_mm_sketch_host -> (mini_x, mini_y, mini_off).  mini_cap None: a minimizer per base (always enough)."""
    text, off = pack_seqs(seqs)
    n = C.c_int64(0)
    moff = np.zeros(len(off), dtype=np.int64)
    L = lib()
    if mini_cap is None:
        mini_cap = len(text)                     # a base ends one minimizer at most
    mx, my = np.zeros(mini_cap, dtype=np.uint64), np.zeros(mini_cap, dtype=np.uint64)
    N.check(L.gbx_mm_sketch_host(C.byref(p), len(off) - 1, N.ptr(text), N.ptr(off), int(rid_ordinal), N.ptr(mx), N.ptr(my), mini_cap, N.ptr(moff),
                                 C.byref(n)))
    return mx[:n.value], my[:n.value], moff


def index_host(p, seqs):
    """gbx_mm_index_build_host -> (keys, key_off, vals, info)"""
    text, off = pack_seqs(seqs)
    cap = max(len(text), 1)
    keys, koff, vals = np.zeros(cap, dtype=np.uint64), np.zeros(cap + 1, dtype=np.int64), np.zeros(cap, dtype=np.uint64)
    st = MmIndexInfo()
    N.check(lib().gbx_mm_index_build_host(C.byref(p), len(off) - 1, N.ptr(text), N.ptr(off), N.ptr(keys), N.ptr(koff), cap, N.ptr(vals), cap, C.byref(st)))
    return keys[:st.n_keys], koff[:st.n_keys + 1], vals[:st.n_vals], st


class DeviceMmIndex:
    """The minimizer index of a reference, resident in HBM.  mini_cap None: room for a minimizer per base (always enough)."""

    def __init__(self, p, seqs, device, stream=None, mini_cap=None):
        import torch
        self.p, self.device = p, device
        check_params(p)
        text, off = pack_seqs(seqs)
        self.n_seqs, self.total_len = len(off) - 1, int(off[-1])
        self.max_len = int(np.diff(off).max()) if self.n_seqs else 0
        self.mini_cap = max(self.total_len, 1) if mini_cap is None else int(mini_cap)
        L = lib()
        self.blob = torch.empty(L.gbx_mm_index_bytes(self.mini_cap), dtype=torch.uint8, device=device)
        self.text = torch.from_numpy(text).to(device)
        self.off = torch.from_numpy(off).to(device)
        wb = L.gbx_mm_index_workspace_bytes(C.byref(p), self.n_seqs, self.total_len, self.mini_cap)
        work = torch.empty(max(wb, 1), dtype=torch.uint8, device=device)
        N.check(L.gbx_mm_index_build_device(C.byref(p), self.n_seqs, self.text.data_ptr(), self.off.data_ptr(), self.total_len,
                                            self.blob.data_ptr(), self.mini_cap, work.data_ptr(), wb, stream))
        self.info = MmIndexInfo()
        N.check(L.gbx_mm_index_stats(self.blob.data_ptr(), self.mini_cap, C.byref(self.info), stream))
        del work

    @property
    def mid_occ(self):
        return self.info.mid_occ

    def flat(self):
        """(keys, key_off, vals) as numpy arrays"""
        c = max(self.mini_cap, 1)
        a256 = lambda v: (v + 255) & ~255
        o_keys, o_koff = 256, 256 + a256(c * 8)
        o_vals = o_koff + a256((c + 1) * 8)
        b = self.blob.cpu().numpy()
        nk, nv = self.info.n_keys, self.info.n_vals
        return (b[o_keys:o_keys + nk * 8].view(np.uint64).copy(), b[o_koff:o_koff + (nk + 1) * 8].view(np.int64).copy(),
                b[o_vals:o_vals + nv * 8].view(np.uint64).copy())


class DeviceMmSeeder(ST.Fits):
    """Reads resident in HBM and everything a seeding call leaves there.  mini_cap / anchor_cap None: a minimizer per base, and
    anchors sized by `anchors_per_mini` of them; counts() reports the need when a capacity was too small."""

    FIT = (("minimizers", 0, "mini_cap"), ("anchors", 1, "anchor_cap"))

    def __init__(self, index, reads, device=None, mini_cap=None, anchor_cap=None, anchors_per_mini=4):
        import torch
        self.index, self.p = index, index.p
        self.device = device = index.device if device is None else device
        text, off = pack_seqs(reads)
        self.n_reads, self.total_len = len(off) - 1, int(off[-1])
        if self.n_reads > MAX_READS:
            raise ValueError("at most %d reads a call" % MAX_READS)
        self.mini_cap = max(self.total_len, 1) if mini_cap is None else int(mini_cap)
        self.anchor_cap = max(self.mini_cap * anchors_per_mini, 1) if anchor_cap is None else int(anchor_cap)
        self.text, self.seq_off = torch.from_numpy(text).to(device), torch.from_numpy(off).to(device)
        e = ST.allocator(device)
        self.mini_x, self.mini_y = e(self.mini_cap, torch.int64), e(self.mini_cap, torch.int64)
        self.mini_off = torch.zeros(self.n_reads + 1, dtype=torch.int64, device=device)
        self.ax, self.ay = e(self.anchor_cap, torch.int64), e(self.anchor_cap, torch.int64)
        self.off = torch.zeros(self.n_reads + 1, dtype=torch.int64, device=device)
        self.hdr = torch.zeros(max(self.n_reads, 1) * N.CHAIN_CALL_DTYPE.itemsize, dtype=torch.uint8, device=device)
        self.rep_len, self.n_mini = e(self.n_reads, torch.int32), e(self.n_reads, torch.int32)
        self.cnt = torch.zeros(2, dtype=torch.int64, device=device)
        self.work_bytes = lib().gbx_mm_seed_workspace_bytes(C.byref(self.p), self.n_reads, self.total_len, self.mini_cap, self.anchor_cap)
        self.work = torch.empty(max(self.work_bytes, 1), dtype=torch.uint8, device=device)

    def run(self, stream=None):
        ix = self.index
        N.check(lib().gbx_mm_seed_device(C.byref(self.p), ix.blob.data_ptr(), ix.mini_cap, ix.n_seqs, ix.max_len, self.n_reads,
                                         self.text.data_ptr(), self.seq_off.data_ptr(), self.total_len, self.mini_x.data_ptr(),
                                         self.mini_y.data_ptr(), self.mini_cap, self.mini_off.data_ptr(), self.ax.data_ptr(), self.ay.data_ptr(),
                                         self.anchor_cap, self.off.data_ptr(), self.hdr.data_ptr(), self.rep_len.data_ptr(),
                                         self.n_mini.data_ptr(), self.cnt.data_ptr(), self.work.data_ptr(), self.work_bytes, stream))

    def counts(self):
        """(minimizers, anchors) of the last run(); anchors -1 when the minimizers did not fit.  Synchronises."""
        c = self.cnt.cpu().numpy()
        return int(c[0]), int(c[1])

    def chain_batch(self):
        """The calls of the last run() as a DeviceChainBatch over the same tensors (no copy).  Reads the anchor count."""
        from .chain import DeviceChainBatch
        self._need_fit()
        return DeviceChainBatch.from_tensors(dict(off=self.off, ax=self.ax, ay=self.ay, hdr=self.hdr), self.device)

    def results(self):
        """dict of numpy arrays, cut to the counts (to the capacities where they were exceeded)"""
        m, a = self.counts()
        m, a = min(max(m, 0), self.mini_cap), min(max(a, 0), self.anchor_cap)
        u = lambda t, n: t[:n].cpu().numpy().view(np.uint64)
        return dict(off=self.off.cpu().numpy(), ax=u(self.ax, a), ay=u(self.ay, a),
                    hdr=self.hdr.cpu().numpy()[:self.n_reads * N.CHAIN_CALL_DTYPE.itemsize].view(N.CHAIN_CALL_DTYPE),
                    rep_len=self.rep_len[:self.n_reads].cpu().numpy(), n_mini=self.n_mini[:self.n_reads].cpu().numpy(),
                    mini_off=self.mini_off.cpu().numpy(), mini_x=u(self.mini_x, m), mini_y=u(self.mini_y, m))


def seed_host(p, index_flat, mid_occ, ref_n_seqs, ref_max_len, reads, anchor_cap):
    """gbx_mm_seed_host on the arrays of index_host -> dict as DeviceMmSeeder.results(), plus counts"""
    keys, koff, vals = index_flat
    text, off = pack_seqs(reads)
    n, mcap = len(off) - 1, max(len(text), 1)
    mx, my, moff = np.zeros(mcap, dtype=np.uint64), np.zeros(mcap, dtype=np.uint64), np.zeros(n + 1, dtype=np.int64)
    ax, ay, aoff = np.zeros(max(anchor_cap, 1), dtype=np.uint64), np.zeros(max(anchor_cap, 1), dtype=np.uint64), np.zeros(n + 1, dtype=np.int64)
    hdr = np.zeros(max(n, 1), dtype=N.CHAIN_CALL_DTYPE)
    rep, nm, cnt = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32), np.zeros(2, dtype=np.int64)
    N.check(lib().gbx_mm_seed_host(C.byref(p), N.ptr(np.ascontiguousarray(keys)), N.ptr(np.ascontiguousarray(koff)), len(keys),
                                   N.ptr(np.ascontiguousarray(vals)), mid_occ, ref_n_seqs, ref_max_len, n, N.ptr(text), N.ptr(off), N.ptr(mx), N.ptr(my),
                                   mcap, N.ptr(moff), N.ptr(ax), N.ptr(ay), anchor_cap, N.ptr(aoff), N.ptr(hdr), N.ptr(rep), N.ptr(nm), N.ptr(cnt)))
    m, a = int(cnt[0]), int(cnt[1])
    return dict(off=aoff, ax=ax[:a], ay=ay[:a], hdr=hdr[:n], rep_len=rep[:n], n_mini=nm[:n], mini_off=moff, mini_x=mx[:m], mini_y=my[:m], counts=(m, a))
