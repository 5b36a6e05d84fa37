"""Whole-seed extension: bwa-mem2's extension caller (mem_chain2aln's left extension on the reversed prefixes, then the right one
with the left score as its h0, each with the band retry) on the GPU through gbx_bsw_extend_seeds_* (include/gbx.h).

A seed is a read ``qer[qoff, qoff+lq)``, its reference window ``ref[roff, roff+rlen)`` and the exact match
``read[qbeg, qbeg+len) ~ win[rbeg, rbeg+len)``.  Results are int32[n, 8] in the order of SEED_RESULT_FIELDS.
"""
import ctypes as C

import numpy as np

from . import _native as N
from .bsw import make_params

SEED_DTYPE = np.dtype([("qoff", "<i8"), ("roff", "<i8"), ("lq", "<i4"), ("rlen", "<i4"), ("qbeg", "<i4"),
                       ("rbeg", "<i4"), ("len", "<i4"), ("pad_", "<i4")])
assert SEED_DTYPE.itemsize == 40
SEED_RESULT_FIELDS = ("score", "truesc", "qb", "qe", "rb", "re", "w", "sc0")


class SeedParams(C.Structure):
    _fields_ = [("bsw", N.BswParams), ("pen_clip5", C.c_int32), ("pen_clip3", C.c_int32), ("max_band_try", C.c_int32),
                ("pad_", C.c_int32)]


_declared = None


def lib():
    """libgbx.so with the seed entries declared (raises if the library or the entries are missing)."""
    global _declared
    L = N.lib()
    if _declared is not L:
        vp, i64, sz = C.c_void_p, C.c_int64, C.c_size_t
        L.gbx_bsw_seed_default_params.argtypes = [C.POINTER(SeedParams)]
        L.gbx_bsw_seed_default_params.restype = None
        L.gbx_bsw_seeds_workspace_bytes.argtypes = [i64, i64, i64]
        L.gbx_bsw_seeds_workspace_bytes.restype = sz
        L.gbx_bsw_extend_seeds_host.argtypes = [C.POINTER(SeedParams), i64, vp, i64, vp, i64, vp, vp]
        L.gbx_bsw_extend_seeds_device.argtypes = [C.POINTER(SeedParams), i64, vp, i64, vp, i64, vp, vp, vp, sz, vp]
        _declared = L
    return L


def make_seed_params(pen_clip5=5, pen_clip3=5, max_band_try=2, **bsw_kw):
    """bwa mem's defaults (pen_clip5 = pen_clip3 = 5, MAX_BAND_TRY = 2); bsw_kw go to bsw.make_params (end_bonus is not read)."""
    p = SeedParams()
    lib().gbx_bsw_seed_default_params(C.byref(p))
    p.bsw = make_params(**bsw_kw)
    p.pen_clip5, p.pen_clip3, p.max_band_try = pen_clip5, pen_clip3, max_band_try
    return p


class SeedBatch:
    """Two byte arenas of base codes 0..4 and a SEED_DTYPE array."""

    def __init__(self, ref, qer, seeds):
        self.ref = np.ascontiguousarray(ref, dtype=np.uint8)
        self.qer = np.ascontiguousarray(qer, dtype=np.uint8)
        self.seeds = np.ascontiguousarray(seeds, dtype=SEED_DTYPE)
        self.n = int(self.seeds.shape[0])

    def take(self, idx):
        """The seeds at `idx` over the same arenas."""
        return SeedBatch(self.ref, self.qer, self.seeds[np.asarray(idx)])

    @staticmethod
    def from_reads(reads, windows, qbeg, rbeg, length):
        """One seed per (read, window) pair of uint8 code arrays; arenas packed end to end."""
        def pack(seqs):
            lens = np.array([len(s) for s in seqs], dtype=np.int64)
            offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64) if len(seqs) else np.zeros(0, np.int64)
            arena = np.concatenate([np.asarray(s, dtype=np.uint8) for s in seqs]) if len(seqs) else np.zeros(0, np.uint8)
            return arena, offs, lens
        qer, qoff, lq = pack(reads)
        ref, roff, rlen = pack(windows)
        s = np.zeros(len(reads), dtype=SEED_DTYPE)
        s["qoff"], s["roff"], s["lq"], s["rlen"] = qoff, roff, lq, rlen
        s["qbeg"], s["rbeg"], s["len"] = qbeg, rbeg, length
        return SeedBatch(ref, qer, s)


def extend_seeds_host(params, batch, out=None):
    """gbx_bsw_extend_seeds_host -> int32[n, 8] (SEED_RESULT_FIELDS)."""
    if out is None:
        out = np.zeros((batch.n, 8), dtype=np.int32)
    N.check(lib().gbx_bsw_extend_seeds_host(C.byref(params), batch.n, N.ptr(batch.ref), batch.ref.size, N.ptr(batch.qer),
                                            batch.qer.size, N.ptr(batch.seeds), N.ptr(out)))
    return out


class DeviceSeedBatch:
    """A SeedBatch resident in HBM as torch tensors, plus the output and workspace buffers."""

    def __init__(self, batch, device):
        import torch
        t = lambda a: torch.from_numpy(a).to(device)
        pad = np.zeros(64, dtype=np.uint8)
        self.device = device
        self.ref_bytes, self.qer_bytes, self.n = batch.ref.size, batch.qer.size, batch.n
        self.ref = t(np.concatenate([batch.ref, pad]))
        self.qer = t(np.concatenate([batch.qer, pad]))
        self.seeds = t(batch.seeds.view(np.uint8).reshape(-1) if batch.n else np.zeros(40, np.uint8))
        self.out = torch.empty((max(self.n, 1), 8), dtype=torch.int32, device=device)
        self.work_bytes = lib().gbx_bsw_seeds_workspace_bytes(self.n, self.ref_bytes, self.qer_bytes)
        self.work = torch.empty(max(self.work_bytes, 1), dtype=torch.uint8, device=device)

    def run(self, params, stream=None):
        """Asynchronous on `stream` (a raw hipStream_t handle or None)."""
        N.check(lib().gbx_bsw_extend_seeds_device(C.byref(params), self.n, self.ref.data_ptr(), self.ref_bytes,
                                                  self.qer.data_ptr(), self.qer_bytes, self.seeds.data_ptr(),
                                                  self.out.data_ptr(), self.work.data_ptr(), self.work_bytes, stream))

    def results(self):
        return self.out[:self.n].cpu().numpy()


def gen_seeds(n, seed, long_frac=0.003, sub_rate=0.02, n_rate=0.01, indel_rate=0.15, max_indel=16, pad=100,
              clip_rate=0.1, zero_rbeg_rate=0.03):
    """Deterministic seeds in the shape bwa mem hands to its extension.  Every read (151 bp; a share `long_frac` of
    1 001..8 192 bp, the row-kernel classes) is cut from a random genome segment that reaches `pad` bases past both ends; its
    window is the segment less a random 0..pad bases on each side, or, with probability `clip_rate` per side, clipped inside
    the read (rbeg < qbeg; rbeg == 0 and a window that ends at the seed's end come up too).  The seed (19..63 bp) sits at the
    read's start, end or a random place in between.  Outside the seed span the read gets a deletion of 1..max_indel bases
    paired with an insertion as long on the same side (read length and seed position stay put; the diagonal moves),
    substitutions and 1 % N."""
    rng = np.random.default_rng(seed)
    lq = np.full(n, 151, dtype=np.int64)
    is_long = rng.random(n) < long_frac
    lq[is_long] = rng.integers(1001, 8193, int(is_long.sum()))
    ln = np.minimum(rng.integers(19, 64, n), lq)
    u = rng.random(n)
    qbeg = np.where(u < 0.2, 0, np.where(u < 0.4, lq - ln, (rng.random(n) * (lq - ln + 1)).astype(np.int64)))
    q0 = qbeg + ln
    # genome segments (their concatenation is the reference arena) and the windows in them
    glen = lq + 2 * pad
    goff = np.concatenate([[0], np.cumsum(glen)[:-1]]).astype(np.int64)
    ref = rng.integers(0, 4, int(glen.sum()), dtype=np.uint8)
    cl = pad - rng.integers(0, pad + 1, n)
    clip = (rng.random(n) < clip_rate) & (qbeg > 0)
    cl = np.where(clip, pad + 1 + (rng.random(n) * qbeg).astype(np.int64), cl)               # window starts inside the read
    cl = np.where((rng.random(n) < zero_rbeg_rate) & (qbeg > 0), pad + qbeg, cl)             # ... right at the seed: rbeg == 0
    we = pad + lq + rng.integers(0, pad + 1, n)
    clip = (rng.random(n) < clip_rate) & (q0 < lq)
    we = np.where(clip, pad + q0 + (rng.random(n) * (lq - q0)).astype(np.int64), we)         # ends inside the read (maybe at q0)
    # reads: segment bases, then the paired indels, then substitutions and N outside the seed
    T = int(lq.sum())
    qo = np.concatenate([[0], np.cumsum(lq)[:-1]]).astype(np.int64)
    read_of = np.repeat(np.arange(n), lq)
    local = np.arange(T, dtype=np.int64) - qo[read_of]
    qer = ref[goff[read_of] + pad + local]
    L = rng.integers(1, max_indel + 1, (2, n))
    ev_l = (rng.random(n) < indel_rate) & (qbeg >= L[0] + 2)
    ev_r = (rng.random(n) < indel_rate) & (lq - q0 >= L[1] + 2)
    L = np.where(np.stack([ev_l, ev_r]), L, 0)
    x_l = (rng.random(n) * (qbeg - L[0] + 1)).astype(np.int64)                  # left deletion [x, x+L) inside [0, qbeg)
    x_r = q0 + (rng.random(n) * (lq - q0 - L[1] + 1)).astype(np.int64)          # right deletion inside [q0, lq)
    starts = np.concatenate([qo + x_l, qo + x_r])
    runs = np.concatenate([L[0], L[1]])
    keep = np.ones(T, dtype=bool)
    keep[np.repeat(starts, runs) + (np.arange(int(runs.sum())) - np.repeat(np.cumsum(runs) - runs, runs))] = False
    qer = qer[keep]
    dropped = L[0] + L[1]
    new_start = qo - (np.cumsum(dropped) - dropped)                              # read starts after the deletions
    y_l = (rng.random(n) * (qbeg - L[0] + 1)).astype(np.int64)                  # left insertion: at or before the seed
    y_r = q0 - L[0] + (rng.random(n) * (lq - q0 - L[1])).astype(np.int64)       # right insertion: after the seed, inside
    at = np.repeat(np.concatenate([new_start + y_l, new_start + y_r]), runs)
    qer = np.insert(qer, at, rng.integers(0, 4, at.size, dtype=np.uint8))
    assert qer.size == T
    outside = (local < qbeg[read_of]) | (local >= q0[read_of])
    sub = outside & (rng.random(T) < sub_rate)
    qer[sub] = (qer[sub] + rng.integers(1, 4, int(sub.sum()), dtype=np.uint8)) % 4
    qer[outside & (rng.random(T) < n_rate)] = 4
    s = np.zeros(n, dtype=SEED_DTYPE)
    s["qoff"], s["lq"], s["qbeg"], s["len"] = qo, lq, qbeg, ln
    s["roff"], s["rlen"], s["rbeg"] = goff + cl, we - cl, pad + qbeg - cl
    return SeedBatch(ref, qer, s)
