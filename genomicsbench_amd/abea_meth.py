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
SITES_COUNT, SITES_FILL = 1, 2                           # GBX_ABEA_METH_SITES_COUNT / _FILL
NO_BAD_JOB = 2 ** 63 - 1                                 # *d_first_bad when every job passes the checks


def _declare(L):
    vp, i64, i32 = N.C.c_void_p, N.C.c_int64, N.C.c_int
    L.gbx_abea_meth_sites_work.argtypes, L.gbx_abea_meth_sites_work.restype = [i64, i64], i64
    L.gbx_abea_meth_sites_device.argtypes = [i32, i64] + [vp] * 11 + [i64, vp, vp, i64, vp, vp]
    L.gbx_abea_meth_tables_host.argtypes = [i64, vp, vp, vp, i64, vp, vp]
    L.gbx_abea_meth_order_work.argtypes, L.gbx_abea_meth_order_work.restype = [i64], i64
    L.gbx_abea_meth_order_device.argtypes = [i64, vp, i64, i64, vp, i64, i32, vp, vp, vp, vp, vp]
    L.gbx_abea_meth_tsv_host.argtypes = [i64, vp, vp, i64] + [vp] * 6 + [i32, i32, i32, i32, i64, vp, vp]


_lib = N.declare_once(_declare)


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


def tables_host(events_per_base, flank_len):
    """gbx_abea_meth_tables_host -> dict(flogsum, trans, pre_flank, post_flank): the half of the plan that needs the host C library"""
    epb = np.ascontiguousarray(events_per_base, np.float64)
    n = len(epb)
    p = dict(flogsum=np.zeros(FLOGSUM_TBL, np.float32), trans=np.zeros((max(n, 1), NTRANS), np.float32),
             pre_flank=np.zeros(max(flank_len, 0), np.float32), post_flank=np.zeros(max(flank_len, 0), np.float32))
    N.check(_lib().gbx_abea_meth_tables_host(n, N.ptr(epb), N.ptr(p["flogsum"]), N.ptr(p["trans"]), flank_len, N.ptr(p["pre_flank"]),
                                             N.ptr(p["post_flank"])))
    return p


def tsv_host(sites, scores, read_names, contig_names, rc, ref_off, ref_len, ref_arena, version=1, clip_start=-1, clip_end=-1, with_header=False,
             cap=None):
    """gbx_abea_meth_tsv_host -> bytes: the lines f5c call-methylation prints for the sites (scores[s] = unmethylated, methylated).
    cap=None sizes first and then calls with exactly that room."""
    sites = np.ascontiguousarray(sites, SITE_DTYPE)
    scores = np.ascontiguousarray(np.asarray(scores, np.float32).reshape(-1))
    n, nr = len(sites), len(read_names)
    assert scores.size == 2 * n and len(contig_names) == nr
    names = (N.C.c_char_p * max(nr, 1))(*[s.encode() if isinstance(s, str) else s for s in read_names])
    contigs = (N.C.c_char_p * max(nr, 1))(*[s.encode() if isinstance(s, str) else s for s in contig_names])
    rc, ref_off = np.ascontiguousarray(rc, np.uint8), np.ascontiguousarray(ref_off, np.int64)
    ref_len, ref_arena = np.ascontiguousarray(ref_len, np.int32), np.ascontiguousarray(ref_arena, np.uint8)
    need = np.zeros(1, np.int64)

    def call(room):
        out = np.zeros(max(room, 1), np.uint8)
        return _lib().gbx_abea_meth_tsv_host(n, N.ptr(sites), N.ptr(scores), nr, names, contigs, N.ptr(rc), N.ptr(ref_off), N.ptr(ref_len), N.ptr(ref_arena),
                                             version, clip_start, clip_end, 1 if with_header else 0, room, N.ptr(out) if room else None, N.ptr(need)), out
    out = N.call_with_room(call, 0 if cap is None else int(cap), need, fixed=cap is not None)
    return out[:int(need[0])].tobytes()


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


    @classmethod
    def from_device(cls, jobs, seq_arena, order, class_off, reads, model, tables, n_jobs):
        """A job set whose jobs, strings and order never were on the host: `jobs` (uint8, 40 n_jobs bytes), `seq_arena` and
        `order` as DeviceAbeaMethSites leaves them, class_off on the host, `reads` as DeviceAbeaCalib.reads(), the CpG model
        (host) and tables_host's dictionary."""
        import torch
        device = jobs.device
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self = cls.__new__(cls)
        self.js, self.n_jobs = None, int(n_jobs)
        self.class_off = np.ascontiguousarray(class_off, np.int64)
        model = np.ascontiguousarray(model, MODEL_DTYPE)
        assert model.size == NMODEL_CPG and self.class_off.size == NCLASS + 1 and int(self.class_off[NCLASS]) == self.n_jobs
        d = dict(jobs=jobs, seq_arena=seq_arena, order=order, model=t(model.view(np.uint8)))
        d.update({k: t(tables[k]) for k in ("flogsum", "trans", "pre_flank", "post_flank")})
        d.update({k: reads[k] for k in ("event_off", "event_mean", "scale", "shift", "var", "log_var")})
        self.d = d
        self.scores = torch.zeros(max(self.n_jobs, 1), dtype=torch.float32, device=device)
        return self


class DeviceAbeaMethSites:
    """The site planner and the job order on the device, behind DeviceAbeaCalib.record(): takes that object's tensors (pos, rc,
    rec_off, rec, event_off) and the reference segments.  count(): the per-read offsets and the strand flags; size(): synchronises,
    brings the two totals and the flags over, raises GBX_ERR_ARG naming the lowest read whose record runs against its strand, and
    allocates; fill(): sites, jobs and strings; order(): the jobs' order, class_off and the per-job checks (synchronises for the
    48 bytes; raises what gbx_abea_meth_plan_host would, naming the lowest bad job).  Nothing else comes to the host."""

    def __init__(self, cal, ref_off, ref_len, ref_arena):
        import torch
        self.torch, self.cal = torch, cal
        dev = self.device = cal.device
        n = self.n_reads = cal.n_reads
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        ref_arena = np.ascontiguousarray(ref_arena, np.uint8)
        self.ref_off, self.ref_len = t(np.ascontiguousarray(ref_off, np.int64)), t(np.ascontiguousarray(ref_len, np.int32))
        self.ref_arena = t(np.concatenate([ref_arena, np.zeros(16, np.uint8)]))
        assert len(ref_len) == n
        z = lambda dt, k: torch.zeros(max(k, 1), dtype=dt, device=dev)
        self.site_off, self.byte_off, self.bad = z(torch.int64, n + 1), z(torch.int64, n + 1), z(torch.uint8, n)
        self.work = z(torch.uint8, int(_lib().gbx_abea_meth_sites_work(n, ref_arena.size)))
        self.n_sites = self.n_bytes = self.n_jobs = 0
        self.sites = self.jobs = self.seq_arena = self.order_ = None
        self.site_cap = self.seq_cap = 0
        self.class_off, self.first_bad = np.zeros(NCLASS + 1, np.int64), NO_BAD_JOB

    def _sites(self, pass_, stream):
        c, p = self.cal, lambda a: a.data_ptr() if a is not None else None
        rec = c.rec if c.rec is not None else self.torch.zeros((1, 2), dtype=self.torch.int32, device=self.device)
        N.check(_lib().gbx_abea_meth_sites_device(pass_, self.n_reads, p(self.ref_off), p(self.ref_len), p(self.ref_arena), p(c.pos), p(c.rc), p(c.rec_off),
                                                  p(rec), p(self.work), p(self.site_off), p(self.byte_off), p(self.bad), self.site_cap, p(self.sites),
                                                  p(self.jobs), self.seq_cap, p(self.seq_arena), stream))

    def count(self, stream=None):
        self._sites(SITES_COUNT, stream)

    def size(self, site_cap=None, seq_cap=None):
        n, torch = self.n_reads, self.torch
        bad = self.bad[:n].cpu().numpy() if n else np.zeros(0, np.uint8)
        if bad.any():
            raise N.GbxError(N.GBX_ERR_ARG, "gbx_abea_meth_sites_device: the record of read %d runs against its strand" % int(np.flatnonzero(bad)[0]))
        self.n_sites, self.n_bytes = (int(self.site_off[n].item()), int(self.byte_off[n].item())) if n else (0, 0)
        self.n_jobs = 2 * self.n_sites
        self.site_cap = self.n_sites if site_cap is None else int(site_cap)
        self.seq_cap = self.n_bytes if seq_cap is None else int(seq_cap)
        self.sites = torch.zeros(max(self.site_cap, 1) * SITE_DTYPE.itemsize, dtype=torch.uint8, device=self.device)
        self.jobs = torch.zeros(max(2 * self.site_cap, 1) * JOB_DTYPE.itemsize, dtype=torch.uint8, device=self.device)
        self.seq_arena = torch.zeros(max(self.seq_cap, 1) + 16, dtype=torch.uint8, device=self.device)

    def fill(self, stream=None):
        if self.n_reads:
            self._sites(SITES_FILL, stream)

    def order(self, flank_len, stream=None):
        """flank_len: as tables_host's (above the largest row count; the largest event count of a read, and one, serves)"""
        torch = self.torch
        nj = self.n_jobs
        bits = max(1, int(flank_len - 1).bit_length())
        self.order_ = torch.zeros(max(nj, 1), dtype=torch.int32, device=self.device)
        work = torch.zeros(max(int(_lib().gbx_abea_meth_order_work(nj)), 1), dtype=torch.uint8, device=self.device)
        tail = torch.zeros(NCLASS + 2, dtype=torch.int64, device=self.device)
        N.check(_lib().gbx_abea_meth_order_device(nj, self.jobs.data_ptr(), self.n_bytes, self.n_reads, self.cal.dss.event_off.data_ptr(), flank_len, bits,
                                                  work.data_ptr(), self.order_.data_ptr(), tail.data_ptr(), tail[NCLASS + 1:].data_ptr(), stream))
        h = tail.cpu().numpy()                                    # synchronises
        self.class_off, self.first_bad = h[:NCLASS + 1].copy(), int(h[NCLASS + 1])
        if self.first_bad != NO_BAD_JOB:
            self.refuse_bad_job()

    def refuse_bad_job(self):
        """raises what gbx_abea_meth_plan_host says of the lowest bad job (that one job comes to the host for the text)"""
        j = self.first_bad
        job = self.jobs[j * JOB_DTYPE.itemsize:(j + 1) * JOB_DTYPE.itemsize].cpu().numpy().view(JOB_DTYPE)
        raise N.GbxError(N.GBX_ERR_UNSUPPORTED if int(job["seq_len"][0]) - KMER + 1 > MAX_KMERS else N.GBX_ERR_ARG,
                         "gbx_abea_meth_order_device: job %d fails the checks of gbx_abea_meth_plan_host: %s" % (j, job[0]))

    def results(self):
        """(sites, jobs, seq_arena) on the host, as sites_host returns them"""
        ns = min(self.n_sites, self.site_cap)
        return (self.sites.cpu().numpy().view(SITE_DTYPE)[:ns], self.jobs.cpu().numpy().view(JOB_DTYPE)[:2 * ns],
                self.seq_arena[:min(self.n_bytes, self.seq_cap)].cpu().numpy())

    def job_set(self, model, tables):
        return DeviceAbeaMethJobSet.from_device(self.jobs, self.seq_arena, self.order_, self.class_off, self.cal.reads(), model, tables, self.n_jobs)
