"""Paired-end: the insert-size estimate, pairing and the pair decision of bwa-mem (mem_pestat, mem_pair and the decision part of
mem_sam_pe) on the GPU through gbx_mem_pair_* (include/gbx.h), the stage between the alignment regions and the CIGAR stage.  Mate
rescue is the stage before it: ``mem_rescue``.

Input: the regs stage's output for 2 n_pairs interleaved reads (read 2p + e is end e of pair p), made with read_id0 =
2 pair_id0.  Output: four PESTAT_DTYPE records (FF, FR, RF, RR), one PAIR_DTYPE record per pair, the regions with the decision's
changes, and the new CIGAR list, which ``mem_cigar`` aligns.  ``sam_fields`` joins the outputs into SAM's paired fields.
"""
import ctypes as C

import numpy as np

from . import _native as N
from .bsw_seeds import SEED_DTYPE
from .mem_cigar import cigar_string
from .mem_regs import FLAG_REPORTED, FLAG_SUPPLEMENTARY, REG_DTYPE, _results
from .mem_stage import CigarList, Regions

PESTAT_DTYPE = np.dtype([("low", "<i4"), ("high", "<i4"), ("failed", "<i4"), ("pad_", "<i4"), ("avg", "<f8"), ("std", "<f8")])
PAIR_DTYPE = np.dtype([("dist", "<i8"), ("score", "<i4"), ("sub", "<i4"), ("n_sub", "<i4"), ("n_cand", "<i4"), ("z0", "<i4"), ("z1", "<i4"),
                       ("q_pe", "<i4"), ("q_se0", "<i4"), ("q_se1", "<i4"), ("paired", "<i4"), ("proper", "<i4"), ("dir", "<i4")])
assert PESTAT_DTYPE.itemsize == 32 and PAIR_DTYPE.itemsize == 56


class PairParams(C.Structure):           # gbx_mem_pair_params
    _fields_ = [("a", C.c_int32), ("b", C.c_int32), ("o_del", C.c_int32), ("e_del", C.c_int32), ("o_ins", C.c_int32),
                ("e_ins", C.c_int32), ("min_seed_len", C.c_int32), ("T", C.c_int32), ("pen_unpaired", C.c_int32), ("max_ins", C.c_int32),
                ("mapq_coef_len", C.c_int32), ("mapq_coef_fac", C.c_float), ("mask_level", C.c_float), ("no_pairing", C.c_int32)]


@N.declare_once
def lib(L):
    """libgbx.so with the paired-end entries declared (raises if the library or the entries are missing)."""
    vp, i64, i32, sz = C.c_void_p, C.c_int64, C.c_int32, C.c_size_t
    L.gbx_mem_pair_default_params.argtypes = [C.POINTER(PairParams)]
    L.gbx_mem_pair_default_params.restype = None
    L.gbx_mem_pair_workspace_bytes.argtypes = [i64, i64, i32]
    L.gbx_mem_pair_workspace_bytes.restype = sz
    L.gbx_mem_pair_device.argtypes = [C.POINTER(PairParams), i64, i64, vp, vp, vp, i64, vp, vp, i64, vp, i64, vp, i64, i32, vp,
                                      vp, vp, vp, vp, vp, vp, i64, vp, vp, sz, vp]
    L.gbx_mem_pair_host.argtypes = [C.POINTER(PairParams), i64, i64, vp, vp, i64, vp, vp, i64, vp, i64, vp, i64, i32, vp,
                                    vp, vp, vp, vp, vp, vp, i64, C.POINTER(i64)]


def make_params(**kw):
    """bwa mem's defaults (a 1, b 4, o_del = o_ins = 6, e_del = e_ins = 1, min_seed_len 19, T 30, pen_unpaired 17, max_ins 10000,
    mapq_coef_len 50, mask_level 0.5, no_pairing 0) with the fields in `kw` replaced; mapq_coef_fac follows mapq_coef_len unless
    it is given."""
    return N.fill_params(PairParams, lib().gbx_mem_pair_default_params, kw, "gbx_mem_pair_params")


def pestat_records(pes):
    """None, or four (low, high, failed, avg, std) / a PESTAT_DTYPE array -> PESTAT_DTYPE[4]."""
    if pes is None:
        return None
    if isinstance(pes, np.ndarray) and pes.dtype == PESTAT_DTYPE:
        out = np.ascontiguousarray(pes)
    else:
        out = np.zeros(4, dtype=PESTAT_DTYPE)
        for d, (low, high, failed, avg, std) in enumerate(pes):
            out[d] = (low, high, failed, 0, avg, std)
    assert len(out) == 4
    return out


def pair_host(params, regs, reg_off, sel_seeds, sel_res, seeds, l_rep, l_pac, contig_off, pair_id0=0, pes_in=None, psel_cap=None):
    """gbx_mem_pair_host -> dict(pes PESTAT_DTYPE[4], pairs PAIR_DTYPE[n_pairs], pregs REG_DTYPE[n_regs], psel_seeds
    SEED_DTYPE[psel_cap], psel_res int32[psel_cap, 8], n_psel).  psel_cap defaults to the number of regions, which always
    suffices; the new list is written up to psel_cap (zeroed seeds with results of all -1 past n_psel)."""
    regs = np.ascontiguousarray(regs, dtype=REG_DTYPE)
    reg_off = np.ascontiguousarray(reg_off, dtype=np.int64)
    sel_seeds = np.ascontiguousarray(sel_seeds, dtype=SEED_DTYPE)
    sel_res = _results(sel_res)
    seeds = np.ascontiguousarray(seeds, dtype=SEED_DTYPE)
    l_rep = np.ascontiguousarray(l_rep, dtype=np.int32)
    contig_off = np.ascontiguousarray(contig_off, dtype=np.int64)
    n_pairs, n_regs, n_sel = (len(reg_off) - 1) // 2, len(regs), len(sel_seeds)
    assert len(reg_off) == 2 * n_pairs + 1 and len(sel_res) == n_sel and len(l_rep) >= 2 * n_pairs
    pcap = n_regs if psel_cap is None else int(psel_cap)
    pes = np.zeros(4, dtype=PESTAT_DTYPE)
    pairs = np.zeros(max(n_pairs, 1), dtype=PAIR_DTYPE)
    pregs = np.zeros(max(n_regs, 1), dtype=REG_DTYPE)
    psel_seeds = np.zeros(max(pcap, 1), dtype=SEED_DTYPE)
    psel_res = np.zeros((max(pcap, 1), 8), dtype=np.int32)
    given = pestat_records(pes_in)
    n = C.c_int64(0)
    keep = np.zeros(1, np.int32)
    N.check(lib().gbx_mem_pair_host(C.byref(params), n_pairs, int(pair_id0), N.ptr(regs) if n_regs else None, N.ptr(reg_off), n_regs,
                                    N.ptr(sel_seeds) if n_sel else None, N.ptr(sel_res) if n_sel else None, n_sel,
                                    N.ptr(seeds) if len(seeds) else None, len(seeds), N.ptr(l_rep) if len(l_rep) else N.ptr(keep),
                                    int(l_pac), len(contig_off) - 1, N.ptr(contig_off), N.ptr(given), N.ptr(pes), N.ptr(pairs),
                                    N.ptr(pregs), N.ptr(psel_seeds), N.ptr(psel_res), pcap, C.byref(n)))
    return dict(pes=pes, pairs=pairs[:n_pairs], pregs=pregs[:n_regs], psel_seeds=psel_seeds[:pcap], psel_res=psel_res[:pcap],
                n_psel=int(n.value))


class DeviceMemPair:
    """gbx_mem_pair_device behind a ``mem_regs.DeviceMemRegs`` or a ``mem_rescue.DeviceMemRescue`` that was made with read_id0 =
    2 * pair_id0 for interleaved reads: that stage's ``regions``, ``cigar_input`` and ``seeds`` records are used where they are.
    run(stream) can be queued behind that stage's run() on the same stream; no count is read on the host.  Its outputs as
    ``mem_stage`` records: ``regions`` (the same list with the decision's changes), ``pairs``, ``cigar_input``
    (``DeviceMemCigar(pair.cigar_input)`` aligns the new list: psel_cap records, the tail being no records), ``batch``."""

    def __init__(self, regs_stage, params=None, pes_in=None, psel_cap=None):
        import torch
        b, rg, sel = regs_stage.batch, regs_stage.regions, regs_stage.cigar_input
        self.batch, self.input, self.sel, self.seeds = b, rg, sel, regs_stage.seeds
        assert b.n_reads % 2 == 0 and rg.read_id0 % 2 == 0, "interleaved pairs, read_id0 = 2 * pair_id0"
        self.params = params or make_params()
        self.pes_in = pestat_records(pes_in)
        self.n_pairs, self.pair_id0 = b.n_reads // 2, rg.read_id0 // 2
        dev = self.device = b.device
        self.psel_cap = int(sel.n if psel_cap is None else psel_cap)
        self.pes = torch.zeros(4 * PESTAT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.pairs = torch.zeros(max(self.n_pairs, 1) * PAIR_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.pregs = torch.zeros(max(rg.cap, 1) * REG_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.psel_seeds = torch.zeros(max(self.psel_cap, 1) * SEED_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.psel_res = torch.full((max(self.psel_cap, 1), 8), -1, dtype=torch.int32, device=dev)
        self.count = torch.zeros(1, dtype=torch.int64, device=dev)
        self.work_bytes = lib().gbx_mem_pair_workspace_bytes(self.n_pairs, rg.cap, self.params.max_ins)
        self.work = torch.empty(max(self.work_bytes, 1), dtype=torch.uint8, device=dev)
        self.regions = Regions(self.pregs, rg.reg_off, rg.count, rg.cap, rg.read_id0)
        self.cigar_input = CigarList(b, self.psel_seeds, self.psel_res, self.psel_cap)

    def run(self, stream=None):
        """Asynchronous on `stream` (a raw hipStream_t handle or None)."""
        b, rg, sel, sd = self.batch, self.input, self.sel, self.seeds
        N.check(lib().gbx_mem_pair_device(
            C.byref(self.params), self.n_pairs, self.pair_id0, rg.regs.data_ptr(), rg.reg_off.data_ptr(), rg.count.data_ptr(), rg.cap,
            sel.seeds.data_ptr(), sel.res.data_ptr(), sel.n, sd.seeds.data_ptr(), sd.cap, sd.l_rep.data_ptr(),
            b.l_pac, b.n_contigs, b.contig_off.data_ptr(), N.ptr(self.pes_in), self.pes.data_ptr(), self.pairs.data_ptr(),
            self.pregs.data_ptr(), self.psel_seeds.data_ptr(), self.psel_res.data_ptr(), self.psel_cap, self.count.data_ptr(),
            self.work.data_ptr(), self.work_bytes, stream))

    def results(self):
        """dict(pes, pairs, pregs, psel_seeds, psel_res, n_psel) of the last run(), the list in full (psel_cap records); raises
        when a stage before it overflowed or psel_cap was too small."""
        n = int(self.count.item())
        if n < 0:
            raise RuntimeError("mem pair: a stage before it overflowed its capacities")
        if n > self.psel_cap:
            raise RuntimeError("mem pair: %d reported regions do not fit psel_cap = %d" % (n, self.psel_cap))
        nr = int(self.input.count.item())
        return dict(pes=self.pes.cpu().numpy().view(PESTAT_DTYPE).copy(),
                    pairs=self.pairs[:self.n_pairs * PAIR_DTYPE.itemsize].cpu().numpy().view(PAIR_DTYPE).copy(),
                    pregs=self.pregs[:nr * REG_DTYPE.itemsize].cpu().numpy().view(REG_DTYPE).copy(),
                    psel_seeds=self.psel_seeds[:self.psel_cap * SEED_DTYPE.itemsize].cpu().numpy().view(SEED_DTYPE).copy(),
                    psel_res=self.psel_res[:self.psel_cap].cpu().numpy(), n_psel=n)


def _ref_len(words):
    return int(sum(int(w) >> 4 for w in words if (int(w) & 15) in (0, 2, 3, 7, 8)))


def sam_fields(pairs, pregs, alns, cigar):
    """SAM's paired fields, host plumbing.  pairs, pregs: a call's output; alns, cigar: what the CIGAR stage made of the new
    list.  One row per reported record in the list's order, and one for a read with nothing reported, in read order:
    (read, flag, rid, pos, mapq, cigar string, rnext, pnext, tlen), positions 0-based, -1 for none.  flag: 0x1, 0x2 from the
    pair's `proper`, 0x40 / 0x80, 0x10 / 0x20 the strand of the record / of the mate's first reported record, 0x4 / 0x8 for an
    end with nothing reported, 0x800.  An unmapped end takes its mate's place and strand.  tlen = -(p0 - p1 + sign(p0 - p1)) with
    pX = pos + (is_rev ? reference length of the CIGAR - 1 : 0), 0 on different contigs or when either end is unmapped."""
    n_reads = 2 * len(pairs)
    recs = [[] for _ in range(n_reads)]
    for g in pregs[(pregs["flag"] & FLAG_REPORTED) != 0]:
        a = alns[int(g["sel"])]
        words = cigar[int(a["cigar_off"]):int(a["cigar_off"]) + int(a["n_cigar"])]
        recs[int(g["read"])].append(dict(rid=int(a["rid"]), pos=int(a["pos"]), rev=int(a["is_rev"]), mapq=int(g["mapq"]),
                                         sup=int(g["flag"]) & FLAG_SUPPLEMENTARY, cigar=cigar_string(words), rlen=_ref_len(words)))
    rows = []
    for r in range(n_reads):
        mate = recs[r ^ 1][0] if recs[r ^ 1] else None
        base = 0x1 | (0x2 if pairs[r >> 1]["proper"] else 0) | (0x80 if r & 1 else 0x40)
        mine = recs[r] or [None]
        for x in mine:
            flag = base
            if x is None:                            # unmapped: the mate's place and strand
                flag |= 0x4
                rid, pos, rev, mapq, cg = (mate["rid"], mate["pos"], mate["rev"], 0, "*") if mate else (-1, -1, 0, 0, "*")
            else:
                rid, pos, rev, mapq, cg = x["rid"], x["pos"], x["rev"], x["mapq"], x["cigar"]
                flag |= x["sup"]
            m = mate if mate else (dict(rid=rid, pos=pos, rev=rev) if x is not None else None)
            if mate is None:
                flag |= 0x8
            flag |= (0x10 if rev else 0) | (0x20 if m and m["rev"] else 0)
            tlen = 0
            if x is not None and mate is not None and x["rid"] == mate["rid"]:
                p0 = x["pos"] + (x["rlen"] - 1 if x["rev"] else 0)
                p1 = mate["pos"] + (mate["rlen"] - 1 if mate["rev"] else 0)
                tlen = -(p0 - p1 + (1 if p0 > p1 else -1 if p0 < p1 else 0))
            rows.append((r, flag, rid, pos, mapq, cg, m["rid"] if m else -1, m["pos"] if m else -1, tlen))
    return rows
