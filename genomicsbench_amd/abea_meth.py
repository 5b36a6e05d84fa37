"""Host mirror of abea's methylation scoring stage (f5c call-methylation: meth_single, R/benchmarks/abea/src/f5c.c:1375-1380).

A job is one profile_hmm_score call (hmm.c:301-727): the forward score of a run of a read's events under a sequence over
A/C/G/M/T.  ``sites_host`` is calculate_methylation_for_read (meth.c:500-658) without the BAM record: it cuts a read's
reference segment into CpG site groups and emits two jobs per site, the unmethylated and the methylated sequence.  The
scores are computed in libgbx.so on the GPU (one device).
"""
import numpy as np

from . import _native as N
from .abea import EVENT_DTYPE, MODEL_DTYPE, PAIR_DTYPE, KMER

JOB_DTYPE = np.dtype([("seq_off", "<i8"), ("rc_off", "<i8"), ("seq_len", "<i4"), ("read", "<i4"), ("event_start", "<i4"),
                      ("event_stop", "<i4"), ("rc", "<i4"), ("flags", "<i4")])                       # gbx_abea_meth_job
SITE_DTYPE = np.dtype([("read", "<i4"), ("start_position", "<i4"), ("end_position", "<i4"), ("n_cpg", "<i4"), ("ctx_off", "<i8"),
                       ("ctx_len", "<i4"), ("pad_", "<i4")])                                         # gbx_abea_meth_site
assert JOB_DTYPE.itemsize == 40 and SITE_DTYPE.itemsize == 32
PRE_CLIP, POST_CLIP = 1, 2                               # HAF_ALLOW_PRE_CLIP, HAF_ALLOW_POST_CLIP (f5cmisc.h:13-17)
NMODEL_CPG, FLOGSUM_TBL, NTRANS, NCLASS, MAX_KMERS = 15625, 16000, 10, 4, 256


def make_cpg_model(level_mean, level_stdv):
    """model_t table of the 5^6 states over A < C < G < M < T with the cached log (model.c:53: a double log stored as float)."""
    m = np.zeros(NMODEL_CPG, dtype=MODEL_DTYPE)
    m["level_mean"] = level_mean
    m["level_stdv"] = level_stdv
    m["level_log_stdv"] = np.log(m["level_stdv"].astype(np.float64)).astype(np.float32)
    return m


class AbeaMethJobSet:
    """Jobs with their strings, the reads they belong to (event means, scalings, events_per_base) and the CpG model."""

    def __init__(self, jobs, seq_arena, event_off, event_mean, scale, shift, var, log_var, events_per_base, model):
        self.jobs = np.ascontiguousarray(jobs, dtype=JOB_DTYPE)
        self.seq_arena = np.ascontiguousarray(seq_arena, dtype=np.uint8)
        self.event_off = np.ascontiguousarray(event_off, dtype=np.int64)          # n_reads + 1
        self.event_mean = np.ascontiguousarray(event_mean, dtype=np.float32)
        self.scale, self.shift, self.var, self.log_var = (np.ascontiguousarray(a, dtype=np.float32) for a in (scale, shift, var, log_var))
        self.events_per_base = np.ascontiguousarray(events_per_base, dtype=np.float64)
        self.model = np.ascontiguousarray(model, dtype=MODEL_DTYPE)
        assert self.model.size == NMODEL_CPG
        self.n_jobs, self.n_reads = len(self.jobs), len(self.scale)

    @property
    def rows(self):
        return np.abs(self.jobs["event_stop"].astype(np.int64) - self.jobs["event_start"]) + 1

    @property
    def n_kmers(self):
        return self.jobs["seq_len"].astype(np.int64) - KMER + 1

    def cells(self):
        """rows x k-mers x 3 states, summed over the jobs (gbx_abea_meth_cells)"""
        v = np.zeros(1, np.int64)
        N.check(N.lib().gbx_abea_meth_cells(self.n_jobs, N.ptr(self.jobs), N.ptr(v)))
        return int(v[0])

    def events_struct(self):
        """the 24-byte event_t array a reference caller holds (only `mean` is read)"""
        ev = np.zeros(max(len(self.event_mean), 1), dtype=EVENT_DTYPE)
        ev["mean"][:len(self.event_mean)] = self.event_mean
        return ev

    def plan(self):
        """gbx_abea_meth_plan_host -> dict(flogsum, trans, pre_flank, post_flank, order, class_off)"""
        flank_len = int(self.rows.max()) + 1 if self.n_jobs else 2
        p = dict(flogsum=np.zeros(FLOGSUM_TBL, np.float32), trans=np.zeros((max(self.n_reads, 1), NTRANS), np.float32),
                 pre_flank=np.zeros(flank_len, np.float32), post_flank=np.zeros(flank_len, np.float32),
                 order=np.zeros(max(self.n_jobs, 1), np.int32), class_off=np.zeros(NCLASS + 1, np.int64))
        N.check(N.lib().gbx_abea_meth_plan_host(self.n_jobs, N.ptr(self.jobs), self.seq_arena.size, self.n_reads, N.ptr(self.event_off),
                                                N.ptr(self.events_per_base), N.ptr(p["flogsum"]), N.ptr(p["trans"]), flank_len,
                                                N.ptr(p["pre_flank"]), N.ptr(p["post_flank"]), N.ptr(p["order"]), N.ptr(p["class_off"])))
        return p


def score_host(js):
    """gbx_abea_meth_score_host -> float32[n_jobs]"""
    scores = np.zeros(max(js.n_jobs, 1), np.float32)
    ev = js.events_struct()
    N.check(N.lib().gbx_abea_meth_score_host(js.n_jobs, N.ptr(js.jobs), N.ptr(js.seq_arena), js.seq_arena.size, js.n_reads, N.ptr(js.event_off),
                                             N.ptr(ev), N.ptr(js.scale), N.ptr(js.shift), N.ptr(js.var), N.ptr(js.log_var),
                                             N.ptr(js.events_per_base), N.ptr(js.model), N.ptr(scores)))
    return scores[:js.n_jobs]


def sites_host(ref_off, ref_len, ref_arena, ref_start_pos, rc, rec_off, rec):
    """gbx_abea_meth_sites_host -> (sites SITE_DTYPE[n], jobs JOB_DTYPE[2n], seq_arena uint8[]): job 2s scores site s
    unmethylated, job 2s + 1 methylated."""
    ref_off, rec_off = np.ascontiguousarray(ref_off, np.int64), np.ascontiguousarray(rec_off, np.int64)
    ref_len, ref_start_pos = np.ascontiguousarray(ref_len, np.int32), np.ascontiguousarray(ref_start_pos, np.int32)
    ref_arena, rc = np.ascontiguousarray(ref_arena, np.uint8), np.ascontiguousarray(rc, np.uint8)
    rec = np.ascontiguousarray(rec, PAIR_DTYPE) if len(rec) else np.zeros(1, PAIR_DTYPE)
    n = len(ref_len)
    ns, nb = np.zeros(1, np.int64), np.zeros(1, np.int64)
    call = lambda cap, sites, jobs, bcap, arena: N.lib().gbx_abea_meth_sites_host(
        n, N.ptr(ref_off), N.ptr(ref_len), N.ptr(ref_arena), N.ptr(ref_start_pos), N.ptr(rc), N.ptr(rec_off), N.ptr(rec), cap, N.ptr(sites),
        N.ptr(jobs), N.ptr(ns), bcap, N.ptr(arena), N.ptr(nb))
    rcode = call(0, None, None, 0, None)                 # sizes first
    if rcode != 0 and not (rcode == N.GBX_ERR_ARG and (ns[0] > 0 or nb[0] > 0)):
        N.check(rcode)
    cap, bcap = int(ns[0]), int(nb[0])
    sites, jobs, arena = np.zeros(max(cap, 1), SITE_DTYPE), np.zeros(max(2 * cap, 1), JOB_DTYPE), np.zeros(max(bcap, 1), np.uint8)
    N.check(call(cap, sites, jobs, bcap, arena))
    return sites[:cap], jobs[:2 * cap], arena[:bcap]


class AbeaMethReadSet:
    """Reads as call-methylation holds them behind align(): an AbeaReadSet (bases, event means, scale, shift), the
    calibrated var / log_var, events_per_base, the strand, the reference segment with its start, the event-alignment record
    (sorted (ref_pos, event index) pairs) and the CpG model."""

    def __init__(self, rs, var, log_var, events_per_base, rc, ref_off, ref_len, ref_arena, ref_start_pos, rec_off, rec, model):
        self.rs = rs
        self.var, self.log_var = np.ascontiguousarray(var, np.float32), np.ascontiguousarray(log_var, np.float32)
        self.events_per_base = np.ascontiguousarray(events_per_base, np.float64)
        self.rc = np.ascontiguousarray(rc, np.uint8)
        self.ref_off, self.ref_len = np.ascontiguousarray(ref_off, np.int64), np.ascontiguousarray(ref_len, np.int32)
        self.ref_arena, self.ref_start_pos = np.ascontiguousarray(ref_arena, np.uint8), np.ascontiguousarray(ref_start_pos, np.int32)
        self.rec_off, self.rec = np.ascontiguousarray(rec_off, np.int64), np.ascontiguousarray(rec, PAIR_DTYPE)
        self.model = np.ascontiguousarray(model, dtype=MODEL_DTYPE)
        self.n_reads = rs.n_reads

    def sites(self):
        return sites_host(self.ref_off, self.ref_len, self.ref_arena, self.ref_start_pos, self.rc, self.rec_off, self.rec)

    def job_set(self, jobs, seq_arena):
        rs = self.rs
        return AbeaMethJobSet(jobs, seq_arena, rs.event_off, rs.event_mean, rs.scale, rs.shift, self.var, self.log_var, self.events_per_base,
                              self.model)


class DeviceAbeaMethJobSet:
    """An AbeaMethJobSet resident in HBM (torch tensors) with its plan and the scores.  `reads` may hand over device tensors
    (event_off, event_mean, scale, shift, and optionally var, log_var) that already live there, as DeviceAbeaSignalSet /
    DeviceAbeaReadSet / DeviceAbeaCalib hold them."""

    def __init__(self, js, device, reads=None):
        import torch
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self.js, self.n_jobs = js, js.n_jobs
        p = js.plan()
        self.class_off = p["class_off"]                                            # stays on the host
        d = dict(jobs=t(js.jobs.view(np.uint8)), seq_arena=t(np.concatenate([js.seq_arena, np.zeros(16, np.uint8)])),
                 var=t(js.var), log_var=t(js.log_var), model=t(js.model.view(np.uint8)), flogsum=t(p["flogsum"]), trans=t(p["trans"]),
                 pre_flank=t(p["pre_flank"]), post_flank=t(p["post_flank"]), order=t(p["order"]))
        if reads is None:
            reads = dict(event_off=t(js.event_off), event_mean=t(np.concatenate([js.event_mean, np.zeros(4, np.float32)])),
                         scale=t(js.scale), shift=t(js.shift))
        d.update({k: reads[k] for k in ("event_off", "event_mean", "scale", "shift")})
        d.update({k: reads[k] for k in ("var", "log_var") if k in reads})          # DeviceAbeaCalib.reads() holds these too
        self.d = d
        self.scores = torch.zeros(max(self.n_jobs, 1), dtype=torch.float32, device=device)

    def run(self, stream=None):
        d = self.d
        N.check(N.lib().gbx_abea_meth_score_device(self.n_jobs, d["jobs"].data_ptr(), d["seq_arena"].data_ptr(), d["event_off"].data_ptr(),
                                                   d["event_mean"].data_ptr(), d["scale"].data_ptr(), d["shift"].data_ptr(),
                                                   d["var"].data_ptr(), d["log_var"].data_ptr(), d["model"].data_ptr(),
                                                   d["flogsum"].data_ptr(), d["trans"].data_ptr(), d["pre_flank"].data_ptr(),
                                                   d["post_flank"].data_ptr(), d["order"].data_ptr(), N.ptr(self.class_off),
                                                   self.scores.data_ptr(), stream))

    def results(self):
        return self.scores[:self.n_jobs].cpu().numpy()

    def cells(self):
        return self.js.cells()
