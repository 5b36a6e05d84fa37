"""abea between align() and the methylation score: host mirror of what f5c runs per read there (scaling_single,
R/benchmarks/abea/src/f5c.c:1262-1330: postalign and recalibrate_model, align.c:550-762; get_event_alignment_record,
meth.c:15-185), and call-methylation from raw signal in one call.  All arithmetic happens in libgbx.so on the GPU (one device).
"""
import numpy as np

from . import _native as N
from .abea import EVENT_DTYPE, MODEL_DTYPE, PAIR_DTYPE, KMER, alignment_arrays
from .abea_meth import SITE_DTYPE, NMODEL_CPG

FAILED_CALIBRATION, FAILED_ALIGNMENT, FAILED_QUALITY_CHK = 1, 2, 4       # read_stat_flag bits (f5c.h:49-51)
PASS_COUNT, PASS_FILL = 1, 2


def _declare(L):
    vp, i64, i32 = N.C.c_void_p, N.C.c_int64, N.C.c_int
    L.gbx_abea_calib_device.argtypes = [i64] + [vp] * 18
    L.gbx_abea_calib_logvar_host.argtypes = [i64, vp, vp, vp]
    L.gbx_abea_calib_host.argtypes = [i64, vp, vp, vp, i64] + [vp] * 15
    L.gbx_abea_event_record_device.argtypes = [i32, i64] + [vp] * 11 + [i64, vp]
    L.gbx_abea_event_record_host.argtypes = [i64] + [vp] * 6 + [i64, vp, vp, vp, i64, vp, vp]
    L.gbx_abea_call_methylation_host.argtypes = [i64] + [vp] * 8 + [i64] + [vp] * 15 + [i64, vp, vp, vp]


_lib = N.declare_once(_declare)


def logvar_host(var64, n_m_state):
    """gbx_abea_calib_logvar_host: (float)log(var64) for the reads recalibration ran on, 0 for the others"""
    var64, n_m_state = np.ascontiguousarray(var64, np.float64), np.ascontiguousarray(n_m_state, np.int32)
    out = np.zeros(max(len(var64), 1), np.float32)
    N.check(_lib().gbx_abea_calib_logvar_host(len(var64), N.ptr(var64), N.ptr(n_m_state), N.ptr(out)))
    return out[:len(var64)]


def calibrate_host(rs, pairs, n_pairs):
    """gbx_abea_calib_host on an AbeaReadSet and what align_host returned for it -> dict(scale, shift, var, log_var, var64, map,
    events_per_base, n_event_alignment, n_m_state, flags); map is int32[len(seq_arena), 2], read r's seq_len[r] - 5 entries at
    seq_off[r]."""
    n = rs.n_reads
    pairs = np.ascontiguousarray(pairs, PAIR_DTYPE) if len(pairs) else np.zeros(2, PAIR_DTYPE)
    n_pairs = np.ascontiguousarray(n_pairs, np.int32) if n else np.zeros(1, np.int32)
    z = lambda dt: np.zeros(max(n, 1), dt)
    o = dict(scale=np.array(rs.scale, np.float32).copy() if n else z(np.float32), shift=np.array(rs.shift, np.float32).copy() if n else z(np.float32),
             var=z(np.float32), log_var=z(np.float32), var64=z(np.float64), map=np.full((max(rs.seq_arena.size, 1), 2), -7, np.int32),
             events_per_base=z(np.float64), n_event_alignment=z(np.int32), n_m_state=z(np.int32), flags=z(np.int32))
    ev = rs.events_struct() if len(rs.event_mean) else np.zeros(1, EVENT_DTYPE)
    N.check(_lib().gbx_abea_calib_host(n, N.ptr(rs.seq_off), N.ptr(rs.seq_len), N.ptr(rs.seq_arena), rs.seq_arena.size, N.ptr(rs.event_off), N.ptr(ev),
                                       N.ptr(rs.model), N.ptr(pairs), N.ptr(n_pairs), N.ptr(o["scale"]), N.ptr(o["shift"]), N.ptr(o["var"]),
                                       N.ptr(o["log_var"]), N.ptr(o["var64"]), N.ptr(o["map"]), N.ptr(o["events_per_base"]),
                                       N.ptr(o["n_event_alignment"]), N.ptr(o["n_m_state"]), N.ptr(o["flags"])))
    return {k: (v if k == "map" else v[:n]) for k, v in o.items()}


def event_record_host(cigar_off, cigar, pos, rc, seq_off, seq_len, map_, flags=None):
    """gbx_abea_event_record_host -> (rec_off int64[n + 1], rec PAIR_DTYPE[]): the record gbx_abea_meth_sites_host consumes"""
    n = len(seq_len)
    cigar_off, seq_off = np.ascontiguousarray(cigar_off, np.int64), np.ascontiguousarray(seq_off, np.int64)
    cigar = np.ascontiguousarray(cigar, np.uint32) if len(cigar) else np.zeros(1, np.uint32)
    pos, seq_len = np.ascontiguousarray(pos, np.int32), np.ascontiguousarray(seq_len, np.int32)
    rc, map_ = np.ascontiguousarray(rc, np.uint8), np.ascontiguousarray(map_, np.int32)
    flags = None if flags is None else np.ascontiguousarray(flags, np.int32)
    rec_off, total = np.zeros(n + 1, np.int64), np.zeros(1, np.int64)

    def call(cap):
        rec = np.zeros(max(cap, 1), PAIR_DTYPE)
        return _lib().gbx_abea_event_record_host(n, N.ptr(cigar_off), N.ptr(cigar), N.ptr(pos), N.ptr(rc), N.ptr(seq_off), N.ptr(seq_len), map_.shape[0],
                                                 N.ptr(map_), N.ptr(flags), N.ptr(rec_off), cap, N.ptr(rec), N.ptr(total)), rec
    rec = N.call_with_room(call, 0, total)                   # sizes first
    return rec_off, rec[:int(total[0])]


def call_methylation_host(ss, cg, site_cap=None):
    """gbx_abea_call_methylation_host on an AbeaSignalSet and the alignments of datagen.gen_abea_cigars (dict: cigar_off, cigar,
    pos, rc, ref_off, ref_len, ref_arena, cpg_model) -> dict(flags, status, scale, shift, var, events_per_base, sites
    SITE_DTYPE[n_sites], scores float32[n_sites, 2]: unmethylated, methylated)."""
    n = ss.n_reads
    cpg = np.ascontiguousarray(cg["cpg_model"], MODEL_DTYPE)
    assert cpg.size == NMODEL_CPG
    cigar_off, cigar, pos, rc, ref_off, ref_len, ref_arena = alignment_arrays(cg)
    z = lambda dt: np.zeros(max(n, 1), dt)
    o = dict(flags=z(np.int32), status=z(np.int32), scale=z(np.float32), shift=z(np.float32), var=z(np.float32), events_per_base=z(np.float64))
    ns = np.zeros(1, np.int64)
    cap = int(site_cap) if site_cap is not None else int(ref_len.sum()) // 12 + 64      # a CpG group per 16 bases of a uniform draw

    def call(cap):
        sites, scores = np.zeros(max(cap, 1), SITE_DTYPE), np.zeros(2 * max(cap, 1), np.float32)
        return _lib().gbx_abea_call_methylation_host(
            n, N.ptr(ss.raw), N.ptr(ss.raw_off), N.ptr(ss.range), N.ptr(ss.digitisation), N.ptr(ss.offset), N.ptr(ss.seq_off), N.ptr(ss.seq_len),
            N.ptr(ss.seq_arena), ss.seq_arena.size, N.ptr(ss.model), N.ptr(cpg), N.ptr(cigar_off), N.ptr(cigar), N.ptr(pos), N.ptr(rc), N.ptr(ref_off),
            N.ptr(ref_len), N.ptr(ref_arena), N.ptr(o["flags"]), N.ptr(o["status"]), N.ptr(o["scale"]), N.ptr(o["shift"]), N.ptr(o["var"]),
            N.ptr(o["events_per_base"]), cap, N.ptr(sites), N.ptr(scores), N.ptr(ns)), (sites, scores)
    sites, scores = N.call_with_room(call, cap, ns, fixed=site_cap is not None)
    k = int(ns[0])
    o = {a: v[:n] for a, v in o.items()}
    o.update(sites=sites[:k], scores=scores[:2 * k].reshape(k, 2))
    return o


class DeviceAbeaCalib:
    """Calibration and record on the buffers DeviceAbeaSignalSet and its align set leave in HBM: no host copy of the events or
    the pairs is made.  run(): calibration; the per-read var64 and M-state counts come to the host for the logarithm.
    record(): count pass, the total comes to the host, fill pass.  reads() is the `reads=` dictionary of DeviceAbeaMethJobSet."""

    def __init__(self, dss, drs, keep, cigar_off, cigar, pos, rc):
        import torch
        self.torch, self.dss, self.drs = torch, dss, drs
        dev = self.device = dss.device
        n = self.n_reads = dss.n_reads
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        z = lambda dt, k=0: torch.zeros(max(n, 1) + k, dtype=dt, device=dev)
        # align() ran over the reads that have events; a read without any has no pairs
        self.n_pairs = z(torch.int32)
        if len(keep):
            self.n_pairs[t(np.asarray(keep, np.int64))] = drs.n_pairs[:len(keep)]
        self.var, self.var64, self.log_var = z(torch.float32), z(torch.float64), z(torch.float32)
        self.events_per_base, self.n_event_alignment, self.n_m_state, self.flags = z(torch.float64), z(torch.int32), z(torch.int32), z(torch.int32)
        nb = dss.seq_arena.numel()
        self.map = torch.zeros((nb, 2), dtype=torch.int32, device=dev)
        self.near = torch.zeros((nb, 2), dtype=torch.int32, device=dev)
        cigar = np.ascontiguousarray(cigar, np.uint32)
        self.cigar_off, self.cigar = t(np.ascontiguousarray(cigar_off, np.int64)), t(np.concatenate([cigar, np.zeros(4, np.uint32)]))
        self.pos, self.rc = t(np.ascontiguousarray(pos, np.int32)), t(np.ascontiguousarray(rc, np.uint8))
        self.rec_off, self.rec, self.n_rec = z(torch.int64, 1), None, 0

    def launch(self, stream=None):
        """the calibration kernel alone (scale and shift are written, never read: it can be repeated)"""
        s, d = self.dss, self.drs
        N.check(_lib().gbx_abea_calib_device(self.n_reads, s.seq_off.data_ptr(), s.seq_len.data_ptr(), s.seq_arena.data_ptr(), s.event_off.data_ptr(),
                                             s.event_mean.data_ptr(), s.model.data_ptr(), d.out.data_ptr(), self.n_pairs.data_ptr(),
                                             s.scale.data_ptr(), s.shift.data_ptr(), self.var.data_ptr(), self.var64.data_ptr(), self.map.data_ptr(),
                                             self.events_per_base.data_ptr(), self.n_event_alignment.data_ptr(), self.n_m_state.data_ptr(),
                                             self.flags.data_ptr(), stream))

    def run(self, stream=None):
        self.launch(stream)
        self.torch.cuda.synchronize()
        n = self.n_reads
        lv = logvar_host(self.var64[:n].cpu().numpy(), self.n_m_state[:n].cpu().numpy())
        self.log_var[:n] = self.torch.from_numpy(lv).to(self.device)

    def _record(self, pass_, stream):
        s = self.dss
        N.check(_lib().gbx_abea_event_record_device(pass_, self.n_reads, self.cigar_off.data_ptr(), self.cigar.data_ptr(), self.pos.data_ptr(),
                                                    self.rc.data_ptr(), s.seq_off.data_ptr(), s.seq_len.data_ptr(), self.map.data_ptr(),
                                                    self.flags.data_ptr(), self.near.data_ptr(), self.rec_off.data_ptr(),
                                                    self.rec.data_ptr() if self.rec is not None else None, self.n_rec, stream))

    def record_count(self, stream=None):
        self._record(PASS_COUNT, stream)

    def record_size(self):
        """after record_count(): synchronises, brings the total over and allocates the record"""
        self.n_rec = int(self.rec_off[self.n_reads].item()) if self.n_reads else 0
        self.rec = self.torch.zeros((max(self.n_rec, 1), 2), dtype=self.torch.int32, device=self.device)

    def record_fill(self, stream=None):
        if self.n_rec:
            self._record(PASS_FILL, stream)

    def record(self, stream=None):
        self.record_count(stream)
        self.record_size()
        self.record_fill(stream)

    def results(self):
        """dict of the per-read calibration on the host, with the map"""
        n = self.n_reads
        h = lambda a: a[:n].cpu().numpy()
        return dict(scale=h(self.dss.scale), shift=h(self.dss.shift), var=h(self.var), log_var=h(self.log_var), var64=h(self.var64),
                    map=self.map.cpu().numpy(), events_per_base=h(self.events_per_base), n_event_alignment=h(self.n_event_alignment),
                    n_m_state=h(self.n_m_state), flags=h(self.flags))

    def record_results(self):
        """(rec_off, rec) on the host: what the site planner takes"""
        return self.rec_off[:self.n_reads + 1].cpu().numpy(), self.rec.cpu().numpy().view(PAIR_DTYPE).reshape(-1)[:self.n_rec]

    def reads(self):
        s = self.dss
        return dict(event_off=s.event_off, event_mean=s.event_mean, scale=s.scale, shift=s.shift, var=self.var, log_var=self.log_var)
