"""Mate rescue: bwa-mem's mem_matesw around ksw_align2 on the GPU through gbx_mem_rescue_* (include/gbx.h), the stage between
the alignment regions and the paired-end stage, and the insert-size estimate alone (gbx_mem_pestat_*), which bwa makes on the
regions before the rescue.

Input: the regs stage's output for 2 n_pairs interleaved reads, made with read_id0 = 2 pair_id0, and four PESTAT_DTYPE records.
Output: the same region lists in the regs stage's shape with the rescued regions added (REG_DTYPE: the regs stage's record with
its last field named csub), the seed records with one more per surviving rescued region, the new CIGAR list, and a STAT_DTYPE
record per pair.  ``DeviceMemRescue`` hands ``mem_pair.DeviceMemPair`` the records a ``DeviceMemRegs`` hands it; ``pipeline``
queues regs -> pestat -> rescue -> pair -> cigar on one stream.
"""
import ctypes as C

import numpy as np

from . import _native as N
from . import mem_pair as MP
from . import mem_regs as MR
from .bsw_seeds import SEED_DTYPE
from .mem_pair import PESTAT_DTYPE, pestat_records
from .mem_regs import _results
from .mem_stage import CigarList, Regions, Seeds

REG_DTYPE = np.dtype([(n if n != "pad_" else "csub", t) for n, t in MR.REG_DTYPE.descr])
STAT_DTYPE = np.dtype([("n_sw", "<i4"), ("n_added", "<i4"), ("n_kept", "<i4"), ("pad_", "<i4")])
assert REG_DTYPE.itemsize == 88 and STAT_DTYPE.itemsize == 16


class RescueParams(C.Structure):         # gbx_mem_rescue_params
    _fields_ = [("a", C.c_int32), ("b", C.c_int32), ("o_del", C.c_int32), ("e_del", C.c_int32), ("o_ins", C.c_int32),
                ("e_ins", C.c_int32), ("min_seed_len", C.c_int32), ("T", C.c_int32), ("pen_unpaired", C.c_int32), ("max_matesw", C.c_int32),
                ("max_chain_gap", C.c_int32), ("mapq_coef_len", C.c_int32), ("mapq_coef_fac", C.c_float), ("mask_level", C.c_float),
                ("mask_level_redun", C.c_float), ("pad_", C.c_int32)]


@N.declare_once
def lib(L):
    """libgbx.so with the mate-rescue entries declared (raises if the library or the entries are missing)."""
    vp, i64, i32, sz = C.c_void_p, C.c_int64, C.c_int32, C.c_size_t
    PP = C.POINTER(MP.PairParams)
    L.gbx_mem_rescue_default_params.argtypes = [C.POINTER(RescueParams)]
    L.gbx_mem_rescue_default_params.restype = None
    L.gbx_mem_pestat_workspace_bytes.argtypes = [i32]
    L.gbx_mem_pestat_workspace_bytes.restype = sz
    L.gbx_mem_pestat_device.argtypes = [PP, i64, vp, vp, vp, i64, i64, vp, vp, sz, vp]
    L.gbx_mem_pestat_host.argtypes = [PP, i64, vp, vp, i64, i64, vp]
    L.gbx_mem_rescue_workspace_bytes.argtypes = [i64, i64, i32]
    L.gbx_mem_rescue_workspace_bytes.restype = sz
    L.gbx_mem_rescue_device.argtypes = [C.POINTER(RescueParams), i64, i64, vp, vp, vp, i64, vp, i64, vp, vp, vp, vp, i64, vp, i64,
                                        i64, i32, vp, vp, vp, i64, vp, vp, vp, i64, vp, vp, vp, i64, vp, vp, vp, sz, vp]
    L.gbx_mem_rescue_host.argtypes = [C.POINTER(RescueParams), i64, i64, vp, vp, i64, vp, i64, vp, vp, vp, vp, i64, vp, i64,
                                      i64, i32, vp, vp, vp, i64, vp, C.POINTER(i64), vp, i64, C.POINTER(i64), vp, vp, i64, C.POINTER(i64), vp]


def make_params(**kw):
    """bwa mem's defaults (a 1, b 4, o_del = o_ins = 6, e_del = e_ins = 1, min_seed_len 19, T 30, pen_unpaired 17, max_matesw 50,
    max_chain_gap 10000, mapq_coef_len 50, mask_level 0.5, mask_level_redun 0.95) with the fields in `kw` replaced; mapq_coef_fac
    follows mapq_coef_len unless it is given."""
    return N.fill_params(RescueParams, lib().gbx_mem_rescue_default_params, kw, "gbx_mem_rescue_params")


def most_added(n_pairs, n_regs, max_matesw):
    """The regions a call can add at most: four per anchor."""
    return 4 * min(int(n_regs), 2 * int(n_pairs) * int(max_matesw))


def pestat_host(pair_params, regs, reg_off, l_pac):
    """gbx_mem_pestat_host -> PESTAT_DTYPE[4]: the estimate gbx_mem_pair_* would make of these regions."""
    regs = np.ascontiguousarray(regs).view(REG_DTYPE)
    reg_off = np.ascontiguousarray(reg_off, dtype=np.int64)
    pes = np.zeros(4, dtype=PESTAT_DTYPE)
    N.check(lib().gbx_mem_pestat_host(C.byref(pair_params), (len(reg_off) - 1) // 2, N.ptr(regs) if len(regs) else None, N.ptr(reg_off),
                                      len(regs), int(l_pac), N.ptr(pes)))
    return pes


def rescue_host(params, regs, reg_off, seeds, l_rep, read_off, read_len, text, qer, l_pac, contig_off, pes, pair_id0=0, xreg_cap=None,
                xseed_cap=None, xsel_cap=None):
    """gbx_mem_rescue_host -> dict(xregs REG_DTYPE[n_xregs], xreg_off, n_xregs, xseeds SEED_DTYPE[xseed_cap], n_xseeds, xsel_seeds
    SEED_DTYPE[xsel_cap], xsel_res int32[xsel_cap, 8], n_xsel, stats STAT_DTYPE[n_pairs]).  The capacities default to what always
    suffices."""
    regs = np.ascontiguousarray(regs).view(REG_DTYPE)
    reg_off = np.ascontiguousarray(reg_off, dtype=np.int64)
    seeds = np.ascontiguousarray(seeds, dtype=SEED_DTYPE)
    l_rep = np.ascontiguousarray(l_rep, dtype=np.int32)
    read_off = np.ascontiguousarray(read_off, dtype=np.int64)
    read_len = np.ascontiguousarray(read_len, dtype=np.int32)
    text = np.ascontiguousarray(text, dtype=np.uint8)
    qer = np.ascontiguousarray(qer, dtype=np.uint8)
    contig_off = np.ascontiguousarray(contig_off, dtype=np.int64)
    pes = pestat_records(pes)
    n_pairs, n_regs, n_seeds = (len(reg_off) - 1) // 2, len(regs), len(seeds)
    assert len(reg_off) == 2 * n_pairs + 1 and min(len(l_rep), len(read_off), len(read_len)) >= 2 * n_pairs
    extra = most_added(n_pairs, n_regs, params.max_matesw)
    rcap = n_regs + extra if xreg_cap is None else int(xreg_cap)
    kcap = n_seeds + extra if xseed_cap is None else int(xseed_cap)
    scap = n_regs + extra if xsel_cap is None else int(xsel_cap)
    xregs = np.zeros(max(rcap, 1), dtype=REG_DTYPE)
    xreg_off = np.zeros(2 * n_pairs + 1, dtype=np.int64)
    xseeds = np.zeros(max(kcap, 1), dtype=SEED_DTYPE)
    xsel_seeds = np.zeros(max(scap, 1), dtype=SEED_DTYPE)
    xsel_res = np.zeros((max(scap, 1), 8), dtype=np.int32)
    stats = np.zeros(max(n_pairs, 1), dtype=STAT_DTYPE)
    nr, nk, ns = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    keep = np.zeros(2, np.int64)
    opt = lambda a: N.ptr(a) if len(a) else N.ptr(keep)
    N.check(lib().gbx_mem_rescue_host(
        C.byref(params), n_pairs, int(pair_id0), N.ptr(regs) if n_regs else None, N.ptr(reg_off), n_regs, N.ptr(seeds) if n_seeds else None,
        n_seeds, opt(l_rep), opt(read_off), opt(read_len), N.ptr(text), len(text), opt(qer), len(qer), int(l_pac), len(contig_off) - 1,
        N.ptr(contig_off), N.ptr(pes), N.ptr(xregs), rcap, N.ptr(xreg_off), C.byref(nr), N.ptr(xseeds), kcap, C.byref(nk), N.ptr(xsel_seeds),
        N.ptr(xsel_res), scap, C.byref(ns), N.ptr(stats)))
    return dict(xregs=xregs[:nr.value], xreg_off=xreg_off, n_xregs=int(nr.value), xseeds=xseeds[:kcap], n_xseeds=int(nk.value),
                xsel_seeds=xsel_seeds[:scap], xsel_res=xsel_res[:scap], n_xsel=int(ns.value), stats=stats[:n_pairs])


class DeviceMemRescue:
    """gbx_mem_pestat_device and gbx_mem_rescue_device behind a ``mem_regs.DeviceMemRegs`` that was made with read_id0 =
    2 * pair_id0 for interleaved reads.  run(stream) queues both behind the regs stage's run(); no count is read on the host.  Its
    outputs as ``mem_stage`` records are a regs stage's: ``regions``, ``seeds`` (with the new seed records), ``cigar_input``,
    ``batch``, and ``pairs`` None, so ``DeviceMemPair(rescue, pes_in=rescue.pes_host(stream))`` follows; that is the one 128-byte
    copy and synchronisation the paired stage's host pointer costs."""
    pairs = None

    def __init__(self, regs_stage, params=None, pair_params=None, pes=None, xreg_cap=None, xseed_cap=None, xsel_cap=None):
        import torch
        b, rg, sd = self.batch, self.input, self.input_seeds = regs_stage.batch, regs_stage.regions, regs_stage.seeds
        assert b.n_reads % 2 == 0 and rg.read_id0 % 2 == 0, "interleaved pairs, read_id0 = 2 * pair_id0"
        self.params = params or make_params()
        self.pair_params = pair_params or MP.make_params()
        self.n_reads, self.read_id0 = b.n_reads, rg.read_id0
        self.n_pairs, self.pair_id0 = b.n_reads // 2, rg.read_id0 // 2
        dev = self.device = b.device
        extra = most_added(self.n_pairs, rg.cap, self.params.max_matesw)
        self.reg_cap = int(rg.cap + extra if xreg_cap is None else xreg_cap)
        self.seed_cap = int(sd.cap + extra if xseed_cap is None else xseed_cap)
        self.sel_cap = int(rg.cap + extra if xsel_cap is None else xsel_cap)
        self.given = pestat_records(pes)
        self.pes = torch.zeros(4 * PESTAT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        if self.given is not None:
            self.pes.copy_(torch.from_numpy(self.given.view(np.uint8).copy()))
        self.regs = torch.zeros(max(self.reg_cap, 1) * REG_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.reg_off = torch.zeros(self.n_reads + 1, dtype=torch.int64, device=dev)
        self.seed_recs = torch.zeros(max(self.seed_cap, 1) * SEED_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.sel_seeds = torch.zeros(max(self.sel_cap, 1) * SEED_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.sel_res = torch.full((max(self.sel_cap, 1), 8), -1, dtype=torch.int32, device=dev)
        self.stats = torch.zeros(max(self.n_pairs, 1) * STAT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.counts = torch.zeros(3, dtype=torch.int64, device=dev)          # regions, reported regions, seed records
        self.work_bytes = lib().gbx_mem_rescue_workspace_bytes(self.n_pairs, rg.cap, self.params.max_matesw)
        self.work = torch.empty(max(self.work_bytes, 1), dtype=torch.uint8, device=dev)
        self.pes_work_bytes = lib().gbx_mem_pestat_workspace_bytes(self.pair_params.max_ins)
        self.pes_work = torch.empty(max(self.pes_work_bytes, 1), dtype=torch.uint8, device=dev)
        self.regions = Regions(self.regs, self.reg_off, self.counts[:1], self.reg_cap, self.read_id0)
        self.seeds = Seeds(self.seed_recs, self.seed_cap, sd.l_rep)
        self.cigar_input = CigarList(b, self.sel_seeds, self.sel_res, self.sel_cap)

    def run(self, stream=None):
        """Asynchronous on `stream` (a raw hipStream_t handle or None)."""
        b, rg, sd = self.batch, self.input, self.input_seeds
        if self.given is None:
            N.check(lib().gbx_mem_pestat_device(C.byref(self.pair_params), self.n_pairs, rg.regs.data_ptr(), rg.reg_off.data_ptr(),
                                                rg.count.data_ptr(), rg.cap, b.l_pac, self.pes.data_ptr(), self.pes_work.data_ptr(),
                                                self.pes_work_bytes, stream))
        c = self.counts.data_ptr()
        N.check(lib().gbx_mem_rescue_device(
            C.byref(self.params), self.n_pairs, self.pair_id0, rg.regs.data_ptr(), rg.reg_off.data_ptr(), rg.count.data_ptr(), rg.cap,
            sd.seeds.data_ptr(), sd.cap, sd.l_rep.data_ptr(), b.read_off.data_ptr(), b.read_len.data_ptr(), b.ref.data_ptr(),
            b.ref_bytes, b.qer.data_ptr(), b.qer_bytes, b.l_pac, b.n_contigs, b.contig_off.data_ptr(), self.pes.data_ptr(),
            self.regs.data_ptr(), self.reg_cap, self.reg_off.data_ptr(), c, self.seed_recs.data_ptr(), self.seed_cap, c + 16,
            self.sel_seeds.data_ptr(), self.sel_res.data_ptr(), self.sel_cap, c + 8, self.stats.data_ptr(), self.work.data_ptr(),
            self.work_bytes, stream))

    def pes_host(self, stream=None):
        """The four records of the last run() as a host array: what the paired stage behind it takes as pes_in.  `stream`: the
        stream run() was queued on (a raw hipStream_t handle or None); the copy is queued on it and it is synchronised, so the
        records are the run's whatever torch's current stream is."""
        out = np.zeros(4, dtype=PESTAT_DTYPE)
        N.check(N.lib().gbx_memcpy_d2h(N.ptr(out), self.pes.data_ptr(), out.nbytes, stream))
        N.check(N.lib().gbx_stream_synchronize(stream))
        return out

    def results(self):
        """dict(pes, xregs, xreg_off, n_xregs, xseeds, n_xseeds, xsel_seeds, xsel_res, n_xsel, stats) of the last run(); raises
        when a stage before it overflowed or a capacity was too small."""
        nr, ns, nk = (int(x) for x in self.counts.cpu().numpy())
        if nr < 0 or ns < 0 or nk < 0:
            raise RuntimeError("mem rescue: a stage before it overflowed its capacities")
        if nr > self.reg_cap or ns > self.sel_cap or nk > self.seed_cap:
            raise RuntimeError("mem rescue: %d regions, %d reported ones and %d seed records do not fit the capacities %d, %d and %d" %
                               (nr, ns, nk, self.reg_cap, self.sel_cap, self.seed_cap))
        return dict(pes=self.pes.cpu().numpy().view(PESTAT_DTYPE).copy(), xregs=self.regs[:nr * REG_DTYPE.itemsize].cpu().numpy().view(REG_DTYPE).copy(),
                    xreg_off=self.reg_off.cpu().numpy(), n_xregs=nr,
                    xseeds=self.seed_recs[:self.seed_cap * SEED_DTYPE.itemsize].cpu().numpy().view(SEED_DTYPE).copy(), n_xseeds=nk,
                    xsel_seeds=self.sel_seeds[:self.sel_cap * SEED_DTYPE.itemsize].cpu().numpy().view(SEED_DTYPE).copy(),
                    xsel_res=self.sel_res[:self.sel_cap].cpu().numpy(), n_xsel=ns,
                    stats=self.stats[:self.n_pairs * STAT_DTYPE.itemsize].cpu().numpy().view(STAT_DTYPE).copy())


def pipeline(ext, stream=None, pair_id0=0, regs_params=None, rescue_params=None, pair_params=None, cigar_params=None, cigar_cap=None,
             z_bytes=None):
    """regs -> pestat -> rescue -> pair -> cigar on one stream behind a ``mem_chain.DeviceSeedExtension`` that has been queued on
    it (``mem_pipeline.Stages`` from "regs" to "cigar").  The estimate is read back once between the rescue and the paired stage
    (128 bytes, one synchronisation): the paired stage takes it as a host pointer.  -> (regs, rescue, pair, cigar) stages, all
    queued; synchronise before results()."""
    from .mem_pipeline import Stages
    caps = {k: v for k, v in (("cigar_cap", cigar_cap), ("z_bytes", z_bytes)) if v is not None}
    st = Stages(ext=ext, id0=pair_id0, params=dict(regs=regs_params, rescue=rescue_params, pair=pair_params, cigar=cigar_params), caps=caps)
    st.queue(stream, "regs", "cigar")
    return st.regs, st.rescue, st.pair, st.cigar
