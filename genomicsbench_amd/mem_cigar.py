"""CIGAR, edit distance and position of extended seeds: bwa-mem's mem_reg2aln / bwa_gen_cigar2 / ksw_global2 on the GPU through
gbx_mem_cigar_* (include/gbx.h), the stage behind the seed extension.

Input: the ``bsw_seeds.SEED_DTYPE`` records of the chaining stage, their extension results (int32[n, 8] in the order of
``bsw_seeds.SEED_RESULT_FIELDS``), the 2 L-byte text (``mem_chain.text_of``) and the reads' arena.
Output: one ALN_DTYPE record per seed (rid -1: no alignment) and the CIGAR words, ``len << 4 | op`` with BAM's op numbers.
"""
import ctypes as C

import numpy as np

from . import _native as N
from .bsw_seeds import SEED_DTYPE
from .mem_chain import one_contig
from .mem_stage import CigarList

ALN_DTYPE = np.dtype([("pos", "<i8"), ("cigar_off", "<i8"), ("rid", "<i4"), ("is_rev", "<i4"), ("n_cigar", "<i4"), ("nm", "<i4"),
                      ("score", "<i4"), ("w", "<i4"), ("tries", "<i4"), ("pad_", "<i4")])
assert ALN_DTYPE.itemsize == 48
RESULT_DTYPE = np.dtype([("score", "<i4"), ("truesc", "<i4"), ("qb", "<i4"), ("qe", "<i4"), ("rb", "<i4"), ("re", "<i4"),
                         ("w", "<i4"), ("sc0", "<i4")])
assert RESULT_DTYPE.itemsize == 32
CIGAR_OPS = "MIDNSHP=X"


class CigarParams(C.Structure):          # gbx_mem_cigar_params
    _fields_ = [("mat", C.c_int32 * 25), ("o_del", C.c_int32), ("e_del", C.c_int32), ("o_ins", C.c_int32), ("e_ins", C.c_int32),
                ("w", C.c_int32)]


@N.declare_once
def lib(L):
    """libgbx.so with the CIGAR entries declared (raises if the library or the entries are missing)."""
    vp, i64, i32, sz = C.c_void_p, C.c_int64, C.c_int32, C.c_size_t
    L.gbx_mem_cigar_default_params.argtypes = [C.POINTER(CigarParams)]
    L.gbx_mem_cigar_default_params.restype = None
    L.gbx_mem_cigar_record_z_bytes.argtypes = [C.POINTER(CigarParams), i32, i32]
    L.gbx_mem_cigar_record_z_bytes.restype = sz
    L.gbx_mem_cigar_workspace_bytes.argtypes = [i64, i64]
    L.gbx_mem_cigar_workspace_bytes.restype = sz
    L.gbx_mem_cigar_device.argtypes = [C.POINTER(CigarParams), i64, vp, vp, vp, i64, vp, i64, i64, i32, vp, vp, vp, i64, vp, vp, sz, vp]
    L.gbx_mem_cigar_host.argtypes = [C.POINTER(CigarParams), i64, vp, vp, vp, i64, vp, i64, i64, i32, vp, vp, vp, i64, C.POINTER(i64)]


def make_params(a=None, b=None, **kw):
    """bwa mem's defaults (match 1, mismatch -4, N -1, o_del = o_ins = 6, e_del = e_ins = 1, w 100) with the fields in `kw`
    replaced; ``a`` / ``b`` rebuild the matrix as bwa_fill_scmat does (match a, mismatch -b, N -1), ``mat`` sets all 25."""
    mat = kw.pop("mat", None)
    p = N.fill_params(CigarParams, lib().gbx_mem_cigar_default_params, kw, "gbx_mem_cigar_params")
    if a is not None or b is not None:
        a, b = (1 if a is None else a), (4 if b is None else b)
        for t in range(5):
            for q in range(5):
                p.mat[t * 5 + q] = -1 if t == 4 or q == 4 else a if t == q else -b
    if mat is not None:
        for i, x in enumerate(np.asarray(mat, dtype=np.int32).reshape(25)):
            p.mat[i] = int(x)
    return p


def cigar_string(words):
    """'5S96M1D50M' from CIGAR words."""
    return "".join("%d%s" % (int(w) >> 4, CIGAR_OPS[int(w) & 15]) for w in np.asarray(words, dtype=np.uint32))


def _results(res):
    r = np.ascontiguousarray(res, dtype=np.int32) if not (isinstance(res, np.ndarray) and res.dtype == RESULT_DTYPE) else res
    return np.ascontiguousarray(r).view(np.int32).reshape(-1, 8)


def cigar_host(params, seeds, res, text, qer, l_pac, contig_off=None, cigar_cap=None):
    """gbx_mem_cigar_host -> (alns ALN_DTYPE[n], cigar uint32[n_cigar]).  Without a capacity the call is repeated with the
    count it reported."""
    seeds = np.ascontiguousarray(seeds, dtype=SEED_DTYPE)
    res = _results(res)
    text = np.ascontiguousarray(text, dtype=np.uint8)
    qer = np.ascontiguousarray(qer, dtype=np.uint8)
    co = np.ascontiguousarray(contig_off if contig_off is not None else one_contig(l_pac), dtype=np.int64)
    n = len(seeds)
    assert len(res) == n
    alns = np.zeros(max(n, 1), dtype=ALN_DTYPE)
    cap = int(cigar_cap) if cigar_cap is not None else max(16, 4 * n)
    nc = C.c_int64(0)
    while True:
        cigar = np.zeros(max(cap, 1), dtype=np.uint32)
        rc = lib().gbx_mem_cigar_host(C.byref(params), n, N.ptr(seeds) if n else None, N.ptr(res) if n else None,
                                      N.ptr(text) if text.size else None, text.size, N.ptr(qer) if qer.size else None, qer.size,
                                      int(l_pac), len(co) - 1, N.ptr(co), N.ptr(alns), N.ptr(cigar), cap, C.byref(nc))
        if rc == -1 and nc.value > cap and cigar_cap is None:
            cap = int(nc.value)
            continue
        N.check(rc)
        return alns[:n], cigar[:nc.value]


class DeviceMemCigar:
    """gbx_mem_cigar_device on a ``mem_stage.CigarList`` (a stage's ``cigar_input``) or behind a
    ``mem_chain.DeviceSeedExtension``, which stands for its own: the seed tensor, result tensor and arenas are used as they are
    (no copy).  run(stream) can be queued behind that stage's run() on the same stream; n defaults to the list's n, so no
    count is needed.  z_bytes: the direction room (default: n records of the longest read against a window as long)."""

    def __init__(self, ext, params=None, n=None, cigar_cap=None, z_bytes=None, max_read_len=151):
        import torch
        lst = self.list = ext if isinstance(ext, CigarList) else ext.cigar_input
        self.batch = lst.batch
        self.params = params or make_params()
        dev = self.device = lst.batch.device
        self.n = int(lst.n if n is None else n)
        assert 0 <= self.n <= lst.n
        self.cigar_cap = int(cigar_cap if cigar_cap is not None else 8 * max(self.n, 1))
        if z_bytes is None:
            z_bytes = self.n * lib().gbx_mem_cigar_record_z_bytes(C.byref(self.params), max_read_len, 2 * max_read_len)
        self.z_bytes = int(z_bytes)
        self.alns = torch.zeros(max(self.n, 1) * ALN_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.cigar = torch.zeros(max(self.cigar_cap, 1), dtype=torch.int32, device=dev)
        self.n_cigar = torch.zeros(1, dtype=torch.int64, device=dev)
        self.work_bytes = lib().gbx_mem_cigar_workspace_bytes(self.n, self.z_bytes)
        self.work = torch.empty(max(self.work_bytes, 1), dtype=torch.uint8, device=dev)

    def run(self, stream=None):
        """Asynchronous on `stream` (a raw hipStream_t handle or None)."""
        lst, b = self.list, self.batch
        N.check(lib().gbx_mem_cigar_device(
            C.byref(self.params), self.n, lst.seeds.data_ptr(), lst.res.data_ptr(), b.ref.data_ptr(), b.ref_bytes, b.qer.data_ptr(),
            b.qer_bytes, b.l_pac, b.n_contigs, b.contig_off.data_ptr(), self.alns.data_ptr(), self.cigar.data_ptr(),
            self.cigar_cap, self.n_cigar.data_ptr(), self.work.data_ptr(), self.work_bytes, stream))

    def results(self):
        """(alns ALN_DTYPE[n], cigar uint32[n_cigar]) of the last run(); raises when cigar_cap was too small."""
        nc = int(self.n_cigar.cpu().numpy()[0])
        if nc > self.cigar_cap:
            raise RuntimeError("mem cigar: %d CIGAR words do not fit the capacity %d" % (nc, self.cigar_cap))
        alns = self.alns[:self.n * ALN_DTYPE.itemsize].cpu().numpy().view(ALN_DTYPE).copy()
        return alns, self.cigar[:nc].cpu().numpy().view(np.uint32).copy()
