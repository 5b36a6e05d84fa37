"""Host mirror of the reference kmer-cnt's minimizer index (R/benchmarks/kmer-cnt with use_minimizers = 1: Flye's
VertexIndex::buildIndexMinimizers, vertex_index.cpp:389-497).  Reads come from kmer.py (``KmerReadSet``, ``encode``,
``read_fasta``).  ``minimizers_host`` / ``index_host`` / ``DeviceKmerIndex`` call libgbx.so; the selection, the sort and the
index are built there on the GPU (include/gbx.h, kmer index section)."""
import ctypes as C

import numpy as np

from . import _native as N
from .kmer import KmerReadSet, encode, kmer_text, read_fasta  # noqa: F401  (the readers belong to this interface too)

MAX_K = 31
MAX_WINDOW = 64
STATS_FIELDS = ("n_chosen", "n_distinct", "repetitive_frequency", "n_repetitive_kmers", "n_repetitive_entries", "n_selected",
                "n_entries", "total_len")


class KmerIndexParams(C.Structure):         # gbx_kmer_index_params
    _fields_ = [("k", C.c_int32), ("window", C.c_int32), ("repeat_rate", C.c_float), ("reserved_", C.c_int32)]


class KmerIndexStats(C.Structure):          # gbx_kmer_index_stats
    _fields_ = [(f, C.c_int64) for f in STATS_FIELDS] + [("mean_frequency", C.c_float), ("reserved_", C.c_int32)]


def _declare(L):
    vp, i64, sz, i32 = C.c_void_p, C.c_int64, C.c_size_t, C.c_int32
    L.gbx_kmer_index_workspace_bytes.argtypes = [i32, i64, i64, i32]
    L.gbx_kmer_index_workspace_bytes.restype = sz
    L.gbx_kmer_minimizers_host.argtypes = [vp, i64, vp, i64, vp, vp, vp, vp, vp, i64, vp]
    L.gbx_kmer_index_host.argtypes = [vp, i64, vp, i64, vp, vp, vp, vp, vp, i64, vp, i64]
    L.gbx_kmer_minimizers_device.argtypes = [vp, i64, vp, vp, vp, i64, vp, vp, vp, i64, vp, vp, sz, vp]
    L.gbx_kmer_index_device.argtypes = [vp, i64, vp, vp, vp, i64, vp, vp, vp, i64, vp, i64, vp, sz, vp]


_lib = N.declare_once(_declare)


def _params(k, window, repeat_rate):
    return KmerIndexParams(int(k), int(window), float(repeat_rate), 0)


def _stats_dict(st):
    d = {f: int(getattr(st, f)) for f in STATS_FIELDS}
    d["mean_frequency"] = np.float32(st.mean_frequency)
    return d


def minimizers_host(reads, k, window, mini_cap=None):
    """gbx_kmer_minimizers_host -> (mini_off int64[n_reads + 1], mini_pos int32[n], mini_rev uint8[n]): read r's minimizer
    positions are mini_pos[mini_off[r] : mini_off[r + 1]], ascending; mini_rev is 1 where the k-mer there is reversed.  Without
    mini_cap the output starts at two positions a window and is resized once to the needed count."""
    p = _params(k, window, 0)
    off = np.zeros(reads.n_reads + 1, dtype=np.int64)
    need = (C.c_int64 * 1)()

    def call(cap):
        pos = np.zeros(cap, dtype=np.int32)
        rev = np.zeros(cap, dtype=np.uint8)
        rc = _lib().gbx_kmer_minimizers_host(C.byref(p), reads.n_reads, N.ptr(reads.enc), reads.enc.size, N.ptr(reads.read_off),
                                             N.ptr(reads.read_len), N.ptr(off), N.ptr(pos), N.ptr(rev), cap, need)
        return rc, (pos, rev)

    cap = int(mini_cap) if mini_cap is not None else 2 * reads.n_positions(k) // (int(window) + 1) + reads.n_reads + 16
    pos, rev = N.call_with_room(call, cap, need, fixed=mini_cap is not None)
    n = min(int(need[0]), pos.size)
    return off, pos[:n], rev[:n]


def index_host(reads, k, window, repeat_rate, kmer_cap=None, pos_cap=None):
    """gbx_kmer_index_host -> (stats dict, kmer uint64[n_selected], off int64[n_selected + 1], pos uint64[n_entries]): the
    kept canonical k-mers in ascending code, k-mer j's global positions pos[off[j] : off[j + 1]] ascending.  Without the
    capacities the outputs start at two positions a window and are resized once to the needed counts."""
    p = _params(k, window, repeat_rate)
    st = KmerIndexStats()
    guess = 2 * reads.n_positions(k) // (int(window) + 1) + reads.n_reads + 16
    caps = [int(kmer_cap) if kmer_cap is not None else guess, int(pos_cap) if pos_cap is not None else guess]
    for attempt in range(2):
        kmer = np.zeros(caps[0], dtype=np.uint64)
        off = np.zeros(caps[0] + 1, dtype=np.int64)
        pos = np.zeros(caps[1], dtype=np.uint64)
        rc = _lib().gbx_kmer_index_host(C.byref(p), reads.n_reads, N.ptr(reads.enc), reads.enc.size, N.ptr(reads.read_off),
                                        N.ptr(reads.read_len), C.byref(st), N.ptr(kmer), N.ptr(off), caps[0], N.ptr(pos), caps[1])
        if rc == N.GBX_ERR_ARG and attempt == 0 and kmer_cap is None and pos_cap is None and \
                (st.n_selected > caps[0] or st.n_entries > caps[1]):
            caps = [max(caps[0], int(st.n_selected)), max(caps[1], int(st.n_entries))]
            continue
        N.check(rc)
        break
    nk, ne = min(int(st.n_selected), caps[0]), min(int(st.n_entries), caps[1])
    return _stats_dict(st), kmer[:nk], off[:nk + 1], pos[:ne]


class DeviceKmerIndex:
    """Device-resident reads + outputs + workspace; run() = one gbx_kmer_index_device call on `stream`, no host
    synchronisation.  The workspace is sized for the reads once (it does not depend on k or the window)."""

    def __init__(self, reads, device, k, window, repeat_rate, kmer_cap=0, pos_cap=0):
        import torch
        self.dev = torch.device(device)
        self.n_reads = reads.n_reads
        self.total_len = reads.n_bases
        self.enc = torch.from_numpy(reads.enc if reads.enc.size else np.zeros(1, dtype=np.uint8)).to(self.dev)
        self.read_off = torch.from_numpy(reads.read_off if reads.n_reads else np.zeros(1, dtype=np.int64)).to(self.dev)
        self.read_len = torch.from_numpy(reads.read_len if reads.n_reads else np.zeros(1, dtype=np.int32)).to(self.dev)
        self.stats = torch.zeros(len(STATS_FIELDS) + 1, dtype=torch.int64, device=self.dev)
        self.work = None
        self.set_params(k, window, repeat_rate, kmer_cap, pos_cap)

    def set_params(self, k, window, repeat_rate, kmer_cap=0, pos_cap=0):
        import torch
        self.params = _params(k, window, repeat_rate)
        self.kmer_cap, self.pos_cap = int(kmer_cap), int(pos_cap)
        self.kmer = torch.zeros(max(self.kmer_cap, 1), dtype=torch.int64, device=self.dev)
        self.off = torch.zeros(self.kmer_cap + 1, dtype=torch.int64, device=self.dev)
        self.pos = torch.zeros(max(self.pos_cap, 1), dtype=torch.int64, device=self.dev)
        wb = _lib().gbx_kmer_index_workspace_bytes(int(k), self.n_reads, self.total_len, 1)
        if wb == 0:
            raise ValueError("kmer index: k = %d outside 1..%d, or 2 x %d bases reach 2^40" % (k, MAX_K, self.total_len))
        if self.work is None or self.work.numel() < wb:
            self.work = None
            self.work = torch.empty(wb, dtype=torch.uint8, device=self.dev)
        self.work_bytes = wb

    def run(self, stream=None):
        N.check(_lib().gbx_kmer_index_device(C.byref(self.params), self.n_reads, self.enc.data_ptr(), self.read_off.data_ptr(),
                                             self.read_len.data_ptr(), self.total_len, self.stats.data_ptr(), self.kmer.data_ptr(),
                                             self.off.data_ptr(), self.kmer_cap, self.pos.data_ptr(), self.pos_cap,
                                             self.work.data_ptr(), self.work_bytes, stream))

    def run_minimizers(self, mini_cap, stream=None):
        """One gbx_kmer_minimizers_device call with room for mini_cap positions (the selection alone, in the same workspace)."""
        import torch
        self.mini_cap = int(mini_cap)
        self.mini_off = torch.zeros(self.n_reads + 1, dtype=torch.int64, device=self.dev)
        self.mini_pos = torch.zeros(max(self.mini_cap, 1), dtype=torch.int32, device=self.dev)
        self.mini_rev = torch.zeros(max(self.mini_cap, 1), dtype=torch.uint8, device=self.dev)
        self.n_mini = torch.zeros(1, dtype=torch.int64, device=self.dev)
        N.check(_lib().gbx_kmer_minimizers_device(C.byref(self.params), self.n_reads, self.enc.data_ptr(), self.read_off.data_ptr(),
                                                  self.read_len.data_ptr(), self.total_len, self.mini_off.data_ptr(),
                                                  self.mini_pos.data_ptr(), self.mini_rev.data_ptr(), self.mini_cap,
                                                  self.n_mini.data_ptr(), self.work.data_ptr(), self.work_bytes, stream))

    def minimizers(self):
        """-> (needed count, mini_off, mini_pos, mini_rev) of the last run_minimizers (cut at its mini_cap)."""
        need = int(self.n_mini.cpu()[0])
        n = max(0, min(need, self.mini_cap))
        return need, self.mini_off.cpu().numpy().copy(), self.mini_pos[:n].cpu().numpy().copy(), self.mini_rev[:n].cpu().numpy().copy()

    def results(self):
        """-> (stats dict, kmer, off, pos) as index_host returns them (cut at the capacities)."""
        raw = self.stats.cpu().numpy()
        st = dict(zip(STATS_FIELDS, (int(v) for v in raw[:len(STATS_FIELDS)])))
        st["mean_frequency"] = raw[len(STATS_FIELDS):].view(np.float32)[0]
        nk = max(0, min(st["n_selected"], self.kmer_cap))
        ne = max(0, min(st["n_entries"], self.pos_cap))
        return (st, self.kmer[:nk].cpu().numpy().view(np.uint64).copy(), self.off[:nk + 1].cpu().numpy().copy(),
                self.pos[:ne].cpu().numpy().view(np.uint64).copy())
