"""Alignment regions, primary marking and mapping quality: the redundancy skip of bwa-mem's mem_chain2aln, mem_sort_dedup_patch
(without mem_patch_reg), mem_mark_primary_se, mem_approx_mapq_se and the region choice of mem_reg2sam on the GPU through
gbx_mem_regs_* (include/gbx.h), the stage between the seed extension and the CIGAR stage.

Input: the chains and ``bsw_seeds.SEED_DTYPE`` records of the chaining stage, the extension's results (int32[n, 8]) and l_rep.
Output: per read its regions (REG_DTYPE) in bwa's output order, and the CIGAR list: the (seed, result) records of the reported
regions, which ``mem_cigar`` aligns.  ``alignments`` joins the two stages' outputs into one row per reported alignment.
"""
import ctypes as C

import numpy as np

from . import _native as N
from .bsw_seeds import SEED_DTYPE
from .mem_chain import CHAIN_DTYPE
from .mem_cigar import cigar_string
from .mem_stage import CigarList, Regions

REG_DTYPE = np.dtype([("rb", "<i8"), ("re", "<i8"), ("seed", "<i8"), ("qb", "<i4"), ("qe", "<i4"), ("read", "<i4"), ("rid", "<i4"),
                      ("score", "<i4"), ("truesc", "<i4"), ("sub", "<i4"), ("sub_n", "<i4"), ("w", "<i4"), ("seedcov", "<i4"),
                      ("seedlen0", "<i4"), ("secondary", "<i4"), ("mapq", "<i4"), ("flag", "<i4"), ("sel", "<i4"), ("pad_", "<i4")])
assert REG_DTYPE.itemsize == 88
FLAG_REPORTED, FLAG_SUPPLEMENTARY = 1, 0x800


class RegsParams(C.Structure):           # gbx_mem_regs_params
    _fields_ = [("a", C.c_int32), ("b", C.c_int32), ("o_del", C.c_int32), ("e_del", C.c_int32), ("o_ins", C.c_int32),
                ("e_ins", C.c_int32), ("w", C.c_int32), ("max_chain_gap", C.c_int32), ("min_seed_len", C.c_int32), ("T", C.c_int32),
                ("mapq_coef_len", C.c_int32), ("mapq_coef_fac", C.c_float), ("mask_level", C.c_float),
                ("mask_level_redun", C.c_float), ("drop_ratio", C.c_float), ("pad_", C.c_int32)]


@N.declare_once
def lib(L):
    """libgbx.so with the region entries declared (raises if the library or the entries are missing)."""
    vp, i64, sz = C.c_void_p, C.c_int64, C.c_size_t
    L.gbx_mem_regs_default_params.argtypes = [C.POINTER(RegsParams)]
    L.gbx_mem_regs_default_params.restype = None
    L.gbx_mem_regs_workspace_bytes.argtypes = [i64, i64]
    L.gbx_mem_regs_workspace_bytes.restype = sz
    L.gbx_mem_regs_device.argtypes = [C.POINTER(RegsParams), i64, i64, vp, vp, i64, vp, vp, vp, i64, vp, vp, vp, i64, vp, vp,
                                      vp, vp, i64, vp, vp, sz, vp]
    L.gbx_mem_regs_host.argtypes = [C.POINTER(RegsParams), i64, i64, vp, i64, vp, vp, i64, vp, vp, vp, i64, vp, C.POINTER(i64),
                                    vp, vp, i64, C.POINTER(i64)]


def make_params(**kw):
    """bwa mem's defaults (a 1, b 4, o_del = o_ins = 6, e_del = e_ins = 1, w 100, max_chain_gap 10000, min_seed_len 19, T 30,
    mapq_coef_len 50, mask_level 0.5, mask_level_redun 0.95, drop_ratio 0.5) with the fields in `kw` replaced; mapq_coef_fac
    follows mapq_coef_len unless it is given."""
    return N.fill_params(RegsParams, lib().gbx_mem_regs_default_params, kw, "gbx_mem_regs_params")


def _results(res):
    return np.ascontiguousarray(np.ascontiguousarray(res).view(np.int32).reshape(-1, 8))


def regs_host(params, chains, chain_off, seeds, res, l_rep, read_id0=0, reg_cap=None, sel_cap=None):
    """gbx_mem_regs_host -> dict(regs REG_DTYPE[n_regs], reg_off int64[n_reads + 1], n_regs, sel_seeds SEED_DTYPE[sel_cap],
    sel_res int32[sel_cap, 8], n_sel).  The capacities default to the number of seeds, which always suffices; the CIGAR list is
    written up to sel_cap (zeroed seeds with results of all -1 past n_sel)."""
    chains = np.ascontiguousarray(chains, dtype=CHAIN_DTYPE)
    chain_off = np.ascontiguousarray(chain_off, dtype=np.int64)
    seeds = np.ascontiguousarray(seeds, dtype=SEED_DTYPE)
    res = _results(res)
    l_rep = np.ascontiguousarray(l_rep, dtype=np.int32)
    n_reads, n = len(chain_off) - 1, len(seeds)
    assert len(res) == n and len(l_rep) >= n_reads
    rcap = n if reg_cap is None else int(reg_cap)
    scap = n if sel_cap is None else int(sel_cap)
    regs = np.zeros(max(rcap, 1), dtype=REG_DTYPE)
    reg_off = np.zeros(n_reads + 1, dtype=np.int64)
    sel_seeds = np.zeros(max(scap, 1), dtype=SEED_DTYPE)
    sel_res = np.zeros((max(scap, 1), 8), dtype=np.int32)
    nr, ns = C.c_int64(0), C.c_int64(0)
    keep = np.zeros(1, np.int32)
    N.check(lib().gbx_mem_regs_host(C.byref(params), n_reads, int(read_id0), N.ptr(chains) if len(chains) else None, len(chains),
                                    N.ptr(chain_off), N.ptr(seeds) if n else None, n, N.ptr(res) if n else None,
                                    N.ptr(l_rep) if len(l_rep) else N.ptr(keep), N.ptr(regs), rcap, N.ptr(reg_off), C.byref(nr),
                                    N.ptr(sel_seeds), N.ptr(sel_res), scap, C.byref(ns)))
    return dict(regs=regs[:nr.value], reg_off=reg_off, n_regs=int(nr.value), sel_seeds=sel_seeds[:scap], sel_res=sel_res[:scap],
                n_sel=int(ns.value))


class DeviceMemRegs:
    """gbx_mem_regs_device behind a ``mem_chain.DeviceSeedExtension``: the chaining's chains, seeds, counts and l_rep and the
    extension's results are used where they are.  run(stream) can be queued behind the extension's run() on the same stream; no
    count is read on the host.  Its outputs as ``mem_stage`` records: ``regions``, ``seeds`` (the chaining's, carried on),
    ``cigar_input`` (``DeviceMemCigar(regs.cigar_input)`` aligns the reported regions: sel_cap records, the tail being no
    records), ``batch``; ``pairs`` is None: the reads are single."""
    pairs = None

    def __init__(self, ext, params=None, read_id0=0, reg_cap=None, sel_cap=None):
        import torch
        self.ext, self.chain, self.batch, self.seeds = ext, ext.chain, ext.batch, ext.seeds
        self.params = params or make_params()
        self.read_id0 = int(read_id0)
        dev = self.device = self.batch.device
        self.n_reads = self.batch.n_reads
        self.seed_cap = int(ext.n)                   # the seeds the extension answered for
        self.reg_cap = int(self.seed_cap if reg_cap is None else reg_cap)
        self.sel_cap = int(self.seed_cap if sel_cap is None else sel_cap)
        self.regs = torch.zeros(max(self.reg_cap, 1) * REG_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.reg_off = torch.zeros(self.n_reads + 1, dtype=torch.int64, device=dev)
        self.sel_seeds = torch.zeros(max(self.sel_cap, 1) * SEED_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.sel_res = torch.full((max(self.sel_cap, 1), 8), -1, dtype=torch.int32, device=dev)
        self.counts = torch.zeros(2, dtype=torch.int64, device=dev)
        self.work_bytes = lib().gbx_mem_regs_workspace_bytes(self.n_reads, self.seed_cap)
        self.work = torch.empty(max(self.work_bytes, 1), dtype=torch.uint8, device=dev)
        self.regions = Regions(self.regs, self.reg_off, self.counts[:1], self.reg_cap, self.read_id0)
        self.cigar_input = CigarList(self.batch, self.sel_seeds, self.sel_res, self.sel_cap)

    def run(self, stream=None):
        """Asynchronous on `stream` (a raw hipStream_t handle or None)."""
        e, ch = self.ext, self.chain
        N.check(lib().gbx_mem_regs_device(
            C.byref(self.params), self.n_reads, self.read_id0, ch.chains.data_ptr(), ch.counts.data_ptr(), ch.chain_cap,
            ch.chain_off.data_ptr(), ch.seeds.data_ptr(), ch.counts.data_ptr() + 8, self.seed_cap, e.out.data_ptr(),
            ch.l_rep.data_ptr(), self.regs.data_ptr(), self.reg_cap, self.reg_off.data_ptr(), self.counts.data_ptr(),
            self.sel_seeds.data_ptr(), self.sel_res.data_ptr(), self.sel_cap, self.counts.data_ptr() + 8, self.work.data_ptr(),
            self.work_bytes, stream))

    def results(self):
        """dict(regs, reg_off, n_regs, sel_seeds, sel_res, n_sel) of the last run(), the CIGAR list in full (sel_cap records);
        raises when the chaining before it overflowed or a capacity was too small."""
        nr, ns = (int(x) for x in self.counts.cpu().numpy())
        if nr < 0 or ns < 0:
            raise RuntimeError("mem regs: the chaining before it overflowed its capacities")
        if nr > self.reg_cap or ns > self.sel_cap:
            raise RuntimeError("mem regs: %d regions and %d reported ones do not fit the capacities %d and %d" %
                               (nr, ns, self.reg_cap, self.sel_cap))
        regs = self.regs[:nr * REG_DTYPE.itemsize].cpu().numpy().view(REG_DTYPE).copy()
        sel_seeds = self.sel_seeds[:self.sel_cap * SEED_DTYPE.itemsize].cpu().numpy().view(SEED_DTYPE).copy()
        return dict(regs=regs, reg_off=self.reg_off.cpu().numpy(), n_regs=nr, sel_seeds=sel_seeds,
                    sel_res=self.sel_res[:self.sel_cap].cpu().numpy(), n_sel=ns)


def alignments(regs, alns, cigar):
    """One row per reported region, in the CIGAR list's order: (read, rid, pos, is_rev, mapq, flag, cigar string, NM).  regs:
    REG_DTYPE records; alns, cigar: what the CIGAR stage made of the CIGAR list.  flag is the SAM flag's part decided here and
    there: 0x10 reverse strand, 0x800 supplementary."""
    rows = []
    for g in regs[(regs["flag"] & FLAG_REPORTED) != 0]:
        a = alns[int(g["sel"])]
        words = cigar[int(a["cigar_off"]):int(a["cigar_off"]) + int(a["n_cigar"])]
        flag = (0x10 if a["is_rev"] else 0) | (int(g["flag"]) & FLAG_SUPPLEMENTARY)
        rows.append((int(g["read"]), int(a["rid"]), int(a["pos"]), int(a["is_rev"]), int(g["mapq"]), flag, cigar_string(words), int(a["nm"])))
    return rows
