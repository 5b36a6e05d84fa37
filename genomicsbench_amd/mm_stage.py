"""What the long-read stage modules (mm_seed, mm_map, mm_align, mm_sam) share: array marshalling, the device allocator, the sizing of a
PAF text, the host build of the rules (libgbx_mm_cpu.so) and the fits() / _need_fit() pair of the stage classes."""
import ctypes as C
import functools
import os

import numpy as np

from . import _native as N

LINE_ROOM = 192                                              # the bytes of a PAF line besides its two names, at most
TAG_ROOM = 96                                                # the bytes the tags NM ms AS nn and cg:Z: add to a line, at most


def c(a, dt):
    return np.ascontiguousarray(a, dtype=dt)


def pad(a):
    """an array with something to point at"""
    return a if len(a) else np.zeros(1, a.dtype)


def pack_seqs(seqs):
    """[bytes or str] -> (uint8 text, int64 offsets)"""
    bs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
    off = np.zeros(len(bs) + 1, dtype=np.int64)
    np.cumsum([len(b) for b in bs], out=off[1:])
    return np.frombuffer(b"".join(bs), dtype=np.uint8).copy(), off


def allocator(device):
    """-> e(n, dtype): an uninitialised device tensor of max(n, 1) elements"""
    import torch
    return lambda n, dt: torch.empty(max(n, 1), dtype=dt, device=device)


def name_room(qnames, tnames):
    """the bytes the two names of a PAF line take, at most ('*' for no target)"""
    return max([len(s) for s in qnames] + [0]) + max([len(s) for s in tnames] + [1])


def text_cap(n_regs, names, tags=False, cigar_words=0):
    """room for the PAF text of n_regs regions whose names take `names` bytes; tags: with the alignment tags, and 11 bytes a CIGAR word"""
    return n_regs * (LINE_ROOM + (TAG_ROOM if tags else 0) + names) + 11 * cigar_words


@functools.lru_cache(maxsize=None)
def twin():
    """libgbx_mm_cpu.so, the host build of the rules, with its entries declared (parameter structs by reference as void *)"""
    T = C.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), "libgbx_mm_cpu.so"))
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    T.gbx_mm_map_cpu.argtypes = [vp, i64] + [vp] * 17
    T.gbx_mm_paf_cpu.argtypes = [i64, vp, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, i64, vp]
    T.gbx_mm_paf_cpu.restype = i64
    T.gbx_mm_align_cpu.argtypes = [vp, i64, i64] + [vp] * 6 + [vp, i64, vp, vp, vp, vp, i64, i64, vp]
    T.gbx_mm_align_cpu_job.argtypes = [vp, vp, i32, vp, i32, i32, C.c_int, C.c_int, vp, vp, i64]
    T.gbx_mm_align_cpu_job.restype = i64
    T.gbx_mm_paf_cigar_cpu.argtypes = [i64, vp, vp, vp, vp, i64, vp, vp, vp, vp, i64, vp, vp, vp, vp, i64, vp]
    T.gbx_mm_paf_cigar_cpu.restype = i64
    T.gbx_mm_sam_cpu.argtypes = [vp, i64] + [vp] * 4 + [i64] + [vp] * 6 + [i64] + [vp] * 5 + [i64, vp, vp]
    T.gbx_mm_sam_cpu.restype = i64
    T.gbx_mm_sam_cpu_lanes.argtypes = [vp, C.c_int] + T.gbx_mm_sam_cpu.argtypes[1:]
    T.gbx_mm_sam_cpu_lanes.restype = i64
    return T


def paf_text(entry, regs, reg_off, qnames, seq_off, rep_len, tnames, tseq_off, cap=None, alns=None, cigar=None, host=True):
    """The marshalling of every PAF text call -> (text bytes, line_off).  regs and alns come as arrays of their record types; alns
    None: the plain entry.  host: a libgbx.so entry (a status, the length through a pointer), else one of twin() (-> the length)."""
    reg_off = c(reg_off, np.int64)
    n = len(reg_off) - 1
    qn, qo = pack_seqs(qnames)
    tn, to = pack_seqs(tnames)
    with_alns = [] if alns is None else [N.ptr(alns), N.ptr(pad(c(cigar, np.uint32))), len(cigar)]
    if cap is None:
        cap = text_cap(len(regs), name_room(qnames, tnames)) if alns is None else text_cap(len(alns), name_room(qnames, tnames), True, len(cigar))
    lines, line_off, nt = np.zeros(max(cap, 1), np.uint8), np.zeros(n + 1, np.int64), C.c_int64(0)
    args = [n, N.ptr(regs), N.ptr(reg_off)] + with_alns + \
           [N.ptr(pad(qn)), N.ptr(qo), N.ptr(c(seq_off, np.int64)), N.ptr(pad(c(rep_len, np.int32))), len(to) - 1, N.ptr(pad(tn)), N.ptr(to),
            N.ptr(c(tseq_off, np.int64)), N.ptr(lines), cap, N.ptr(line_off)]
    if host:
        N.check(entry(*args, C.byref(nt)))
        return lines[:nt.value].tobytes(), line_off
    return lines[:entry(*args)].tobytes(), line_off


class Fits:
    """fits() and _need_fit() of a stage class from FIT, its rows (what, index into counts(), the attribute with the capacity).  A
    count without a capacity has no row and is not compared."""
    FIT = ()

    def _fit(self):
        cnt = self.counts()
        return cnt, all(0 <= cnt[i] <= getattr(self, cap) for _, i, cap in self.FIT)

    def fits(self):
        return self._fit()[1]

    def _need_fit(self):
        """counts(), or GBX_ERR_ARG where one does not fit its capacity"""
        cnt, ok = self._fit()
        if not ok:
            got = ["%d %s" % (cnt[i], what) for what, i, _ in self.FIT]
            raise N.GbxError(N.GBX_ERR_ARG, "%s and %s do not fit %s" % (", ".join(got[:-1]), got[-1],
                                                                          ", ".join("%s = %d" % (cap, getattr(self, cap)) for _, _, cap in self.FIT)))
        return cnt
