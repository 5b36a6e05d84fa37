"""abea eventalign: host mirror of what f5c eventalign runs per read behind the calibration (realign_read,
R/benchmarks/abea/src/eventalign.c:1263-1540 with its Viterbi profile HMM, :345-911), the summary and the TSV of its records
(:1580-1642, :1651-1662, :1853-1938), and eventalign from raw signal in one call.  The alignment happens in libgbx.so on the
GPU (one device); the summary and the TSV are host code of the library.
"""
import numpy as np

from . import _native as N
from .abea import EVENT_DTYPE, MODEL_DTYPE, alignment_arrays as _cg

REC_DTYPE = np.dtype([("ref_pos", "<i4"), ("event_idx", "<i4"), ("state", "<i4")])          # gbx_abea_eventalign_rec
SUMMARY_DTYPE = np.dtype([("num_events", "<i4"), ("num_steps", "<i4"), ("num_stays", "<i4"), ("num_skips", "<i4"), ("sum_duration", "<f8"),
                          ("sum_z_score", "<f8"), ("reference_span", "<i4"), ("pad_", "<i4")])
ROWS_CAP, NTRANS = 1024, 10
ST_ROWS, ST_UNDEFINED, ST_BOUND = 1, 2, 4
STATE_M, STATE_B = ord("M"), ord("B")

_lib = N.lib


def trans_host(events_per_base):
    """gbx_abea_eventalign_trans_host: float32[n, 10], the transition logarithms of every read"""
    epb = np.ascontiguousarray(events_per_base, np.float64)
    out = np.zeros((max(len(epb), 1), NTRANS), np.float32)
    N.check(_lib().gbx_abea_eventalign_trans_host(len(epb), N.ptr(epb), N.ptr(out)))
    return out[:len(epb)]


def eventalign_host(seq_off, seq_len, event_off, events, model, calib, cg, region=(-1, -1)):
    """gbx_abea_eventalign_host.  events: EVENT_DTYPE[]; calib: what abea_calib.calibrate_host returned (scale, shift, var, log_var,
    events_per_base, map, flags); cg: dict(cigar_off, cigar, pos, rc, ref_off, ref_len, ref_arena) as datagen.gen_abea_cigars gives
    -> dict(rec REC_DTYPE[n_events]: read r's records at event_off[r] - event_off[0], n_rec, status)."""
    n = len(seq_len)
    seq_off, seq_len = np.ascontiguousarray(seq_off, np.int64), np.ascontiguousarray(seq_len, np.int32)
    event_off = np.ascontiguousarray(event_off, np.int64)
    events = np.ascontiguousarray(events, EVENT_DTYPE) if len(events) else np.zeros(1, EVENT_DTYPE)
    model = np.ascontiguousarray(model, MODEL_DTYPE)
    map_ = np.ascontiguousarray(calib["map"], np.int32)
    f = lambda k: np.ascontiguousarray(calib[k], np.float32)
    scale, shift, var, log_var = f("scale"), f("shift"), f("var"), f("log_var")
    epb = np.ascontiguousarray(calib["events_per_base"], np.float64)
    flags = None if calib.get("flags") is None else np.ascontiguousarray(calib["flags"], np.int32)
    cigar_off, cigar, pos, rc, ref_off, ref_len, ref = _cg(cg)
    total = int(event_off[n] - event_off[0]) if n else 0
    rec, n_rec, status = np.zeros(max(total, 1), REC_DTYPE), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    N.check(_lib().gbx_abea_eventalign_host(n, N.ptr(seq_off), N.ptr(seq_len), map_.shape[0], N.ptr(event_off), N.ptr(events), N.ptr(model), N.ptr(scale),
                                            N.ptr(shift), N.ptr(var), N.ptr(log_var), N.ptr(epb), N.ptr(map_), N.ptr(flags), N.ptr(cigar_off), N.ptr(cigar),
                                            N.ptr(pos), N.ptr(rc), N.ptr(ref_off), N.ptr(ref_len), N.ptr(ref), int(region[0]), int(region[1]), N.ptr(rec),
                                            N.ptr(n_rec), N.ptr(status)))
    return dict(rec=rec[:total], n_rec=n_rec[:n], status=status[:n])


def read_records(o, event_off, r):
    """the records of read r out of what eventalign_host / DeviceAbeaEventalign.results / eventalign_from_signal_host returned"""
    a = int(event_off[r] - event_off[0])
    return o["rec"][a:a + int(o["n_rec"][r])]


def summary(event_off, events, model, scale, shift, var, cg, o):
    """gbx_abea_eventalign_summary_host -> SUMMARY_DTYPE[n_reads] (the NM tag is the caller's)"""
    event_off = np.ascontiguousarray(event_off, np.int64)
    n = len(event_off) - 1
    events = np.ascontiguousarray(events, EVENT_DTYPE) if len(events) else np.zeros(1, EVENT_DTYPE)
    model = np.ascontiguousarray(model, MODEL_DTYPE)
    f = lambda a: np.ascontiguousarray(a, np.float32)
    scale, shift, var = f(scale), f(shift), f(var)
    _, _, pos, rc, ref_off, ref_len, ref = _cg(cg)
    rec = np.ascontiguousarray(o["rec"], REC_DTYPE) if len(o["rec"]) else np.zeros(1, REC_DTYPE)
    n_rec = np.ascontiguousarray(o["n_rec"], np.int32)
    out = np.zeros(max(n, 1), SUMMARY_DTYPE)
    N.check(_lib().gbx_abea_eventalign_summary_host(n, N.ptr(event_off), N.ptr(events), N.ptr(model), N.ptr(scale), N.ptr(shift), N.ptr(var), N.ptr(rc),
                                                    N.ptr(pos), N.ptr(ref_off), N.ptr(ref_len), N.ptr(ref), N.ptr(rec), N.ptr(n_rec), N.ptr(out)))
    return out[:n]


def tsv(events, model, scale, shift, var, rc, pos, ref, rec, header=False, print_read_names=False, scale_events=False, write_samples=False,
        read_index=0, read_name=b"", ref_name=b"contig", sample_rate=4000.0):
    """gbx_abea_eventalign_tsv_host for one read -> bytes: emit_event_alignment_tsv's lines, behind the header line if asked for.
    events: the read's own EVENT_DTYPE[]; ref: the read's reference segment (bytes or uint8[]), which starts at pos."""
    events = np.ascontiguousarray(events, EVENT_DTYPE) if len(events) else np.zeros(1, EVENT_DTYPE)
    n_events = len(events)
    model = np.ascontiguousarray(model, MODEL_DTYPE)
    ref = np.frombuffer(bytes(ref), np.uint8) if isinstance(ref, (bytes, bytearray)) else np.ascontiguousarray(ref, np.uint8)
    ref_len = len(ref)
    if not ref_len:
        ref = np.zeros(1, np.uint8)
    rec = np.ascontiguousarray(rec, REC_DTYPE)
    n_rec = len(rec)
    if not n_rec:
        rec = np.zeros(1, REC_DTYPE)
    need = np.zeros(1, np.int64)
    cap = 160 + 128 * n_rec + (len(ref_name) + len(read_name)) * n_rec

    def call(cap):
        text = np.zeros(max(cap, 1), np.uint8)
        return _lib().gbx_abea_eventalign_tsv_host(N.ptr(events), n_events, N.ptr(model), float(scale), float(shift), float(var), int(rc), int(pos),
                                                   N.ptr(ref), ref_len, N.ptr(rec), n_rec, int(header), int(print_read_names), int(scale_events),
                                                   int(write_samples), int(read_index), bytes(read_name), bytes(ref_name), float(sample_rate),
                                                   N.ptr(text), cap, N.ptr(need)), text
    text = N.call_with_room(call, cap, need)
    return text[:int(need[0])].tobytes()


def eventalign_from_signal_host(ss, cg, region=(-1, -1), event_cap=None):
    """gbx_abea_eventalign_from_signal_host on an AbeaSignalSet and the alignments of datagen.gen_abea_cigars -> dict(flags, status,
    scale, shift, var, log_var, events_per_base, event_off, events, rec, n_rec, ea_status)."""
    n = ss.n_reads
    cigar_off, cigar, pos, rc, ref_off, ref_len, ref = _cg(cg)
    z = lambda dt, k=0: np.zeros(max(n, 1) + k, dt)
    o = dict(flags=z(np.int32), status=z(np.int32), scale=z(np.float32), shift=z(np.float32), var=z(np.float32), log_var=z(np.float32),
             events_per_base=z(np.float64), n_rec=z(np.int32), ea_status=z(np.int32))
    event_off, total = z(np.int64, 1), np.zeros(1, np.int64)
    cap = int(event_cap) if event_cap is not None else int(ss.raw_off[-1] - ss.raw_off[0]) // 4 + n + 16

    def call(cap):
        events, rec = np.zeros(max(cap, 1), EVENT_DTYPE), np.zeros(max(cap, 1), REC_DTYPE)
        return _lib().gbx_abea_eventalign_from_signal_host(
            n, N.ptr(ss.raw), N.ptr(ss.raw_off), N.ptr(ss.range), N.ptr(ss.digitisation), N.ptr(ss.offset), N.ptr(ss.seq_off), N.ptr(ss.seq_len),
            N.ptr(ss.seq_arena), ss.seq_arena.size, N.ptr(ss.model), N.ptr(cigar_off), N.ptr(cigar), N.ptr(pos), N.ptr(rc), N.ptr(ref_off), N.ptr(ref_len),
            N.ptr(ref), int(region[0]), int(region[1]), N.ptr(o["flags"]), N.ptr(o["status"]), N.ptr(o["scale"]), N.ptr(o["shift"]), N.ptr(o["var"]),
            N.ptr(o["log_var"]), N.ptr(o["events_per_base"]), N.ptr(event_off), N.ptr(events), cap, N.ptr(total), N.ptr(rec), N.ptr(o["n_rec"]),
            N.ptr(o["ea_status"])), (events, rec)
    events, rec = N.call_with_room(call, cap, total, fixed=event_cap is not None)
    k = int(total[0])
    o = {a: v[:n] for a, v in o.items()}
    o.update(event_off=event_off[:n + 1], events=events[:k], rec=rec[:k])
    return o


class DeviceAbeaEventalign:
    """eventalign on the buffers DeviceAbeaSignalSet and DeviceAbeaCalib leave in HBM, behind cal.run() and cal.record_count() (the
    count pass writes the nearest-k-mer table): no host copy of the events, the map or the pairs is made.  The transition
    logarithms are taken on the host from the per-read events_per_base (80 bytes per read go back up); the order of the reads
    (longest first) is an argsort on the device."""

    def __init__(self, cal, ref_off, ref_len, ref_arena, region=(-1, -1), rows_cap=ROWS_CAP, counts=False):
        torch = self.torch = cal.torch
        self.cal, self.region, self.rows_cap = cal, region, int(rows_cap)
        dev = self.device = cal.device
        n = self.n_reads = cal.n_reads
        s = cal.dss
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.ref_off, self.ref_len = t(np.ascontiguousarray(ref_off, np.int64)), t(np.ascontiguousarray(ref_len, np.int32))
        self.ref = t(np.concatenate([np.ascontiguousarray(ref_arena, np.uint8), np.zeros(16, np.uint8)]))
        self.n_cigar = int(cal.cigar.numel()) - 4
        self.trans = t(trans_host(cal.events_per_base[:n].cpu().numpy()) if n else np.zeros((1, NTRANS), np.float32))
        n_ev = s.event_off[1:n + 1] - s.event_off[:n]
        self.order = torch.argsort(n_ev, descending=True, stable=True).to(torch.int32) if n else torch.zeros(1, dtype=torch.int32, device=dev)
        self.rec = torch.zeros((max(s.n_events_total, 1), 3), dtype=torch.int32, device=dev)
        self.n_rec, self.status = torch.zeros(max(n, 1), dtype=torch.int32, device=dev), torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        self.counts = torch.zeros((max(n, 1), 3), dtype=torch.int64, device=dev) if counts else None
        self.work_bytes = int(_lib().gbx_abea_eventalign_workspace_bytes(n, self.n_cigar, self.rows_cap))
        self.work = torch.zeros(self.work_bytes, dtype=torch.uint8, device=dev)

    def run(self, stream=None):
        c, s = self.cal, self.cal.dss
        N.check(_lib().gbx_abea_eventalign_device(
            self.n_reads, s.seq_off.data_ptr(), s.seq_len.data_ptr(), s.event_off.data_ptr(), s.event_mean.data_ptr(), s.model.data_ptr(),
            s.scale.data_ptr(), s.shift.data_ptr(), c.var.data_ptr(), c.log_var.data_ptr(), self.trans.data_ptr(), c.map.data_ptr(), c.near.data_ptr(),
            c.flags.data_ptr(), c.cigar_off.data_ptr(), c.cigar.data_ptr(), c.pos.data_ptr(), c.rc.data_ptr(), self.ref_off.data_ptr(),
            self.ref_len.data_ptr(), self.ref.data_ptr(), int(self.region[0]), int(self.region[1]), self.order.data_ptr(), self.rec.data_ptr(),
            self.n_rec.data_ptr(), self.status.data_ptr(), self.counts.data_ptr() if self.counts is not None else None, self.n_cigar, self.rows_cap,
            self.work.data_ptr(), self.work_bytes, stream))

    def results(self):
        """dict(rec, n_rec, status) on the host, as eventalign_host returns it"""
        n, k = self.n_reads, self.cal.dss.n_events_total
        return dict(rec=self.rec.cpu().numpy().view(REC_DTYPE).reshape(-1)[:k], n_rec=self.n_rec[:n].cpu().numpy(), status=self.status[:n].cpu().numpy())
