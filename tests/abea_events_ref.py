"""CPU restatement of abea's signal stage (tests/abea_events_ref.c) behind numpy arrays.  Test infrastructure.

The C file states the contract from the reference's lines (f5c.c:1227-1231, events.c:292-503, align.c:49-97); it is built
here on first use, next to this file or, where that is not writable, in a temporary directory.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from genomicsbench_amd.abea import EVENT_DTYPE

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


def _L():
    global _lib
    if _lib is None:
        src = os.path.join(_HERE, "abea_events_ref.c")
        out = os.path.join(_HERE, "libabea_events_ref.so")
        if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
            if not os.access(_HERE, os.W_OK):
                out = os.path.join(tempfile.mkdtemp(prefix="abea_events_ref"), "libabea_events_ref.so")
            subprocess.run(["gcc", "-O2", "-std=c11", "-ffp-contract=off", "-fopenmp", "-fPIC", "-shared", src, "-o", out, "-lm"], check=True)
        _lib = C.CDLL(out)
        vp, i64 = C.c_void_p, C.c_int64
        _lib.aer_detect_many.argtypes = [i64] + [vp] * 8 + [C.c_int]
        _lib.aer_detect_many.restype = None
        _lib.aer_scalings_many.argtypes = [i64] + [vp] * 8 + [C.c_int]
        _lib.aer_scalings_many.restype = None
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def detect(raw, raw_off, range_, digitisation, offset, threads=4):
    """-> (event_off int64[n + 1], events EVENT_DTYPE[total], status int32[n]: 1 where the read has no events)"""
    raw = np.ascontiguousarray(raw, np.int16); raw_off = np.ascontiguousarray(raw_off, np.int64)
    rg, dg, of = (np.ascontiguousarray(a, np.float32) for a in (range_, digitisation, offset))
    n = len(raw_off) - 1
    n_ev = np.zeros(max(n, 1), np.int64)
    L = _L()
    L.aer_detect_many(n, _p(raw), _p(raw_off), _p(rg), _p(dg), _p(of), _p(n_ev), None, None, threads)
    off = np.zeros(n + 1, np.int64); np.cumsum(n_ev[:n], out=off[1:])
    ev = np.zeros(max(int(off[-1]), 1), dtype=EVENT_DTYPE)
    L.aer_detect_many(n, _p(raw), _p(raw_off), _p(rg), _p(dg), _p(of), _p(n_ev), _p(off), _p(ev), threads)
    return off, ev[:int(off[-1])], (n_ev[:n] == 0).astype(np.int32)


def scalings(seq_off, seq_len, seq_arena, event_off, events, model, threads=4):
    """-> (scale, shift) float32[n]"""
    n = len(seq_len)
    seq_off = np.ascontiguousarray(seq_off, np.int64); seq_len = np.ascontiguousarray(seq_len, np.int32)
    ev = np.ascontiguousarray(events) if len(events) else np.zeros(1, EVENT_DTYPE)
    scale, shift = np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.float32)
    _L().aer_scalings_many(n, _p(seq_off), _p(seq_len), _p(seq_arena), _p(np.ascontiguousarray(event_off, np.int64)), _p(ev),
                           _p(np.ascontiguousarray(model)), _p(scale), _p(shift), threads)
    return scale[:n], shift[:n]


def run(ss, threads=4):
    """an AbeaSignalSet -> dict(event_off, events, status, scale, shift)"""
    off, ev, st = detect(ss.raw, ss.raw_off, ss.range, ss.digitisation, ss.offset, threads)
    sc, sh = scalings(ss.seq_off, ss.seq_len, ss.seq_arena, off, ev, ss.model, threads)
    return dict(event_off=off, events=ev, status=st, scale=sc, shift=sh)
