"""Seed chaining between the suffix-array lookup and the seed extension: bwa-mem's mem_chain, mem_chain_flt and the window of
mem_chain2aln on the GPU through gbx_mem_chain_* (include/gbx.h).

Input: per read its SMEMs (``fmi.smem_host`` / ``DeviceFmi.run``) and their hits (``fmi.sal_host`` / ``DeviceFmi.sal``).
Output: the kept chains (CHAIN_DTYPE), ``chain_off`` per read, ``l_rep`` per read, and one ``bsw_seeds.SEED_DTYPE`` record
per seed of every kept chain, in the form gbx_bsw_extend_seeds_* takes: the reference arena is ``text_of(genome)`` (genome +
reverse complement, what ``fmi.build_index`` indexes), the query arena the reads' ``enc``.
"""
import ctypes as C

import numpy as np

from . import _native as N
from .bsw_seeds import SEED_DTYPE
from .fmi import SMEM_DTYPE
from .mem_stage import Batch, CigarList, Seeds

CHAIN_DTYPE = np.dtype([("pos", "<i8"), ("seed_off", "<i8"), ("rmax0", "<i8"), ("rmax1", "<i8"), ("read", "<i4"),
                        ("contig", "<i4"), ("n_seeds", "<i4"), ("weight", "<i4"), ("kept", "<i4"), ("pad_", "<i4")])
assert CHAIN_DTYPE.itemsize == 56


class ChainParams(C.Structure):          # gbx_mem_chain_params
    _fields_ = [("w", C.c_int32), ("max_chain_gap", C.c_int32), ("max_occ", C.c_int32), ("min_seed_len", C.c_int32),
                ("min_chain_weight", C.c_int32), ("max_chain_extend", C.c_int32), ("mask_level", C.c_float),
                ("drop_ratio", C.c_float), ("a", C.c_int32), ("o_del", C.c_int32), ("e_del", C.c_int32), ("o_ins", C.c_int32),
                ("e_ins", C.c_int32), ("pad_", C.c_int32)]


@N.declare_once
def lib(L):
    """libgbx.so with the chaining entries declared (raises if the library or the entries are missing)."""
    vp, i64, i32, sz = C.c_void_p, C.c_int64, C.c_int32, C.c_size_t
    L.gbx_mem_chain_default_params.argtypes = [C.POINTER(ChainParams)]
    L.gbx_mem_chain_default_params.restype = None
    L.gbx_mem_chain_workspace_bytes.argtypes = [i64, i64, i64]
    L.gbx_mem_chain_workspace_bytes.restype = sz
    L.gbx_mem_chain_device.argtypes = ([C.POINTER(ChainParams), i64, vp, vp, i64, vp, vp, vp, i64, vp, vp, vp, i64, i32, vp,
                                        vp, i64, vp, vp, i64, vp, vp, vp, vp, sz, vp])
    L.gbx_mem_chain_host.argtypes = ([C.POINTER(ChainParams), i64, vp, i64, vp, vp, i64, vp, vp, vp, i64, i32, vp,
                                      vp, i64, vp, vp, i64, vp, C.POINTER(i64), C.POINTER(i64)])


def make_params(**kw):
    """bwa mem's defaults (w 100, max_chain_gap 10000, max_occ 500, min_seed_len 19, min_chain_weight 0, max_chain_extend 2^30,
    mask_level = drop_ratio = 0.5, a 1, o_del = o_ins = 6, e_del = e_ins = 1) with the fields in `kw` replaced."""
    return N.fill_params(ChainParams, lib().gbx_mem_chain_default_params, kw, "gbx_mem_chain_params")


def text_of(genome):
    """The 2 L-byte text the hits' coordinates refer to: the genome's base codes, then its reverse complement."""
    g = np.ascontiguousarray(genome, dtype=np.uint8)
    return np.concatenate([g, (3 - g[::-1]).astype(np.uint8)])


def one_contig(genome_len):
    return np.array([0, int(genome_len)], dtype=np.int64)


def chain_host(params, smems, smem_off, pos, pos_off, reads, l_pac, contig_off=None, chain_cap=None, seed_cap=None):
    """gbx_mem_chain_host -> dict(chains CHAIN_DTYPE, chain_off int64[n_reads + 1], seeds SEED_DTYPE, l_rep int32[n_reads]).
    reads: an FmiReadSet (read_off, read_len).  Without capacities the call is repeated with the counts it reported."""
    smems = np.ascontiguousarray(smems, dtype=SMEM_DTYPE)
    smem_off = np.ascontiguousarray(smem_off, dtype=np.int64)
    pos = np.ascontiguousarray(pos, dtype=np.int64)
    pos_off = np.ascontiguousarray(pos_off, dtype=np.int64)
    co = np.ascontiguousarray(contig_off if contig_off is not None else one_contig(l_pac), dtype=np.int64)
    n_reads = reads.n_reads
    chain_off = np.zeros(n_reads + 1, dtype=np.int64)
    l_rep = np.zeros(max(n_reads, 1), dtype=np.int32)
    ccap = int(chain_cap) if chain_cap is not None else max(16, 4 * n_reads)
    scap = int(seed_cap) if seed_cap is not None else max(16, 8 * n_reads)
    nc, ns = C.c_int64(0), C.c_int64(0)
    while True:
        chains = np.zeros(max(ccap, 1), dtype=CHAIN_DTYPE)
        seeds = np.zeros(max(scap, 1), dtype=SEED_DTYPE)
        rc = lib().gbx_mem_chain_host(C.byref(params), n_reads, N.ptr(smems) if len(smems) else None, len(smems), N.ptr(smem_off),
                                      N.ptr(pos) if len(pos) else None, len(pos), N.ptr(pos_off), N.ptr(reads.read_off),
                                      N.ptr(reads.read_len), int(l_pac), len(co) - 1, N.ptr(co), N.ptr(chains), ccap,
                                      N.ptr(chain_off), N.ptr(seeds), scap, N.ptr(l_rep), C.byref(nc), C.byref(ns))
        if rc == -1 and (nc.value > ccap or ns.value > scap) and (chain_cap is None or nc.value <= ccap) and \
                (seed_cap is None or ns.value <= scap):
            ccap, scap = max(ccap, int(nc.value)), max(scap, int(ns.value))
            continue
        N.check(rc)
        return dict(chains=chains[:nc.value], chain_off=chain_off, seeds=seeds[:ns.value], l_rep=l_rep[:n_reads])


class DeviceMemChain:
    """Output and workspace tensors of gbx_mem_chain_device behind a DeviceFmi that has run() and sal(): run(stream) chains
    the SMEMs and hits the DeviceFmi holds in HBM, with their counts read on the device - no host round trip in between.
    ``seeds`` (uint8 tensor of seed_cap SEED_DTYPE records, zeroed past the count) goes to the extension as it is:
    ``extension(text)`` wraps it with the arenas."""

    def __init__(self, dfmi, l_pac, contig_off=None, params=None, chain_cap=None, seed_cap=None):
        import torch
        self.fmi = dfmi
        self.params = params or make_params()
        dev = dfmi.dindex.device
        self.device = dev
        self.l_pac = int(l_pac)
        co = np.ascontiguousarray(contig_off if contig_off is not None else one_contig(l_pac), dtype=np.int64)
        self.n_contigs = len(co) - 1
        self.contig_off = torch.from_numpy(co).to(dev)
        self.n_reads = dfmi.n_reads
        self.chain_cap = int(chain_cap if chain_cap is not None else dfmi.pos_cap)
        self.seed_cap = int(seed_cap if seed_cap is not None else dfmi.pos_cap)
        self.chains = torch.zeros(max(self.chain_cap, 1) * CHAIN_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.seeds = torch.zeros(max(self.seed_cap, 1) * SEED_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.chain_off = torch.zeros(self.n_reads + 1, dtype=torch.int64, device=dev)
        self.l_rep = torch.zeros(max(self.n_reads, 1), dtype=torch.int32, device=dev)
        self.counts = torch.zeros(2, dtype=torch.int64, device=dev)
        self.work_bytes = lib().gbx_mem_chain_workspace_bytes(self.n_reads, dfmi.out_cap, dfmi.pos_cap)
        self.work = torch.empty(max(self.work_bytes, 1), dtype=torch.uint8, device=dev)

    def run(self, stream=None):
        """Asynchronous on `stream` (a raw hipStream_t handle or None)."""
        f = self.fmi
        N.check(lib().gbx_mem_chain_device(
            C.byref(self.params), self.n_reads, f.out.data_ptr(), f.n_out.data_ptr(), f.out_cap, f.smem_off.data_ptr(),
            f.pos.data_ptr(), f.n_pos.data_ptr(), f.pos_cap, f.pos_off.data_ptr(), f.read_off.data_ptr(), f.read_len.data_ptr(),
            self.l_pac, self.n_contigs, self.contig_off.data_ptr(), self.chains.data_ptr(), self.chain_cap,
            self.chain_off.data_ptr(), self.seeds.data_ptr(), self.seed_cap, self.l_rep.data_ptr(), self.counts.data_ptr(),
            self.counts.data_ptr() + 8, self.work.data_ptr(), self.work_bytes, stream))

    def results(self):
        """dict(chains, chain_off, seeds, l_rep) of the last run(); raises when a capacity was too small."""
        nc, ns = (int(x) for x in self.counts.cpu().numpy())
        if nc > self.chain_cap or ns > self.seed_cap:
            raise RuntimeError("mem chain: %d chains and %d seeds do not fit the capacities %d and %d" %
                               (nc, ns, self.chain_cap, self.seed_cap))
        chains = self.chains[:nc * CHAIN_DTYPE.itemsize].cpu().numpy().view(CHAIN_DTYPE).copy()
        seeds = self.seeds[:ns * SEED_DTYPE.itemsize].cpu().numpy().view(SEED_DTYPE).copy()
        return dict(chains=chains, chain_off=self.chain_off.cpu().numpy(), seeds=seeds, l_rep=self.l_rep[:self.n_reads].cpu().numpy())

    def extension(self, text, n=None):
        """A DeviceSeedExtension over this object's seed tensor (no copy), the text as reference arena and the DeviceFmi's reads
        as query arena.  n: how many seed records to extend; default seed_cap (the records past the count are no seeds and
        come back as -1), so that it can be queued behind run() without knowing the count."""
        return DeviceSeedExtension(self, text, self.seed_cap if n is None else int(n))


class DeviceSeedExtension:
    """gbx_bsw_extend_seeds_device on a DeviceMemChain's seed tensor: run(seed_params, stream), results().  It owns the padded
    arenas, so it makes the ``mem_stage.Batch`` the later stages carry on; ``seeds`` and ``cigar_input`` are the chaining's
    seed records, the latter with this object's results."""

    def __init__(self, chain, text, n):
        import torch
        from . import bsw_seeds as BS
        self._bs = BS
        dev = chain.device
        self.chain, self.n = chain, int(n)
        assert 0 <= self.n <= chain.seed_cap
        t = text if isinstance(text, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(text, dtype=np.uint8))
        self.ref_bytes = int(t.numel())
        self.ref = torch.cat([t.to(dev), torch.zeros(64, dtype=torch.uint8, device=dev)])
        enc = chain.fmi.enc
        self.qer_bytes = int(enc.numel())
        self.qer = torch.cat([enc, torch.zeros(64, dtype=torch.uint8, device=dev)])
        self.out = torch.empty((max(self.n, 1), 8), dtype=torch.int32, device=dev)
        self.work_bytes = BS.lib().gbx_bsw_seeds_workspace_bytes(self.n, self.ref_bytes, self.qer_bytes)
        self.work = torch.empty(max(self.work_bytes, 1), dtype=torch.uint8, device=dev)
        f = chain.fmi
        self.batch = Batch(dev, chain.n_reads, self.qer, self.qer_bytes, f.read_off, f.read_len, self.ref, self.ref_bytes, chain.l_pac,
                           chain.n_contigs, chain.contig_off)
        self.seeds = Seeds(chain.seeds, chain.seed_cap, chain.l_rep)
        self.cigar_input = CigarList(self.batch, chain.seeds, self.out, self.n)

    def run(self, seed_params, stream=None):
        N.check(self._bs.lib().gbx_bsw_extend_seeds_device(C.byref(seed_params), self.n, self.ref.data_ptr(), self.ref_bytes,
                                                           self.qer.data_ptr(), self.qer_bytes, self.chain.seeds.data_ptr(),
                                                           self.out.data_ptr(), self.work.data_ptr(), self.work_bytes, stream))

    def results(self, n=None):
        return self.out[:self.n if n is None else n].cpu().numpy()
