"""abea from raw signal: host mirror of what f5c runs per read before align() (event_single, R/benchmarks/abea/src/f5c.c:1219-1242).

ADC counts -> pA -> scrappie's event detection -> method-of-moments scalings, and the chain into the existing align path.
All arithmetic happens in libgbx.so on the GPU (one device).
"""
import numpy as np

from . import _native as N
from .abea import EVENT_DTYPE, MODEL_DTYPE, PAIR_DTYPE, AbeaReadSet, DeviceAbeaReadSet

EV_NONE, EV_INORDER, EV_OVERFLOW = 1, 2, 4           # status bits (include/gbx.h)
PASS_COUNT, PASS_FILL = 1, 2


class AbeaSignalSet:
    """Reads as the sequencer and the basecaller hand them over: int16 samples with their three scaling floats, bases, the pore model."""

    def __init__(self, raw, raw_off, range_, digitisation, offset, seq_off, seq_len, seq_arena, model):
        self.raw = np.ascontiguousarray(raw, dtype=np.int16)
        self.raw_off = np.ascontiguousarray(raw_off, dtype=np.int64)              # n_reads + 1
        self.range = np.ascontiguousarray(range_, dtype=np.float32)
        self.digitisation = np.ascontiguousarray(digitisation, dtype=np.float32)
        self.offset = np.ascontiguousarray(offset, dtype=np.float32)
        self.seq_off = np.ascontiguousarray(seq_off, dtype=np.int64)
        self.seq_len = np.ascontiguousarray(seq_len, dtype=np.int32)
        self.seq_arena = np.ascontiguousarray(seq_arena, dtype=np.uint8)
        self.model = np.ascontiguousarray(model, dtype=MODEL_DTYPE)
        self.n_reads = len(self.seq_len)

    @property
    def n_samples(self):
        return np.diff(self.raw_off)

    def take(self, idx):
        """the reads idx (any order) as a set of their own"""
        idx = np.asarray(idx, dtype=np.int64)
        ns = self.n_samples[idx]
        off = np.zeros(len(idx) + 1, dtype=np.int64); np.cumsum(ns, out=off[1:])
        raw = np.concatenate([self.raw[self.raw_off[i]:self.raw_off[i + 1]] for i in idx] + [np.zeros(0, np.int16)])
        return AbeaSignalSet(raw, off, self.range[idx], self.digitisation[idx], self.offset[idx], self.seq_off[idx], self.seq_len[idx],
                             self.seq_arena, self.model)

    def read_set(self, event_off, event_mean, scale, shift, keep=None):
        """the AbeaReadSet align() takes, of the reads `keep` (default: those that have events)"""
        n_ev = np.diff(event_off)
        if keep is None:
            keep = np.flatnonzero(n_ev > 0)
        off = np.zeros(len(keep) + 1, dtype=np.int64); np.cumsum(n_ev[keep], out=off[1:])
        means = np.concatenate([event_mean[event_off[r]:event_off[r + 1]] for r in keep] + [np.zeros(0, np.float32)])
        return AbeaReadSet(self.seq_off[keep], self.seq_len[keep], self.seq_arena, off, means, scale[keep], shift[keep], self.model), keep


def _cap(ss, cap):
    return int(cap) if cap is not None else int(ss.raw_off[-1] - ss.raw_off[0]) // 4 + ss.n_reads + 16


def events_host(ss, event_cap=None):
    """gbx_abea_events_host -> (event_off int64[n_reads + 1], events EVENT_DTYPE[total], status int32[n_reads])."""
    n = ss.n_reads
    n_ev, off, status = np.zeros(max(n, 1), np.int64), np.zeros(n + 1, np.int64), np.zeros(max(n, 1), np.int32)
    total = np.zeros(1, np.int64)

    def call(cap):
        ev = np.zeros(max(cap, 1), dtype=EVENT_DTYPE)
        return N.lib().gbx_abea_events_host(n, N.ptr(ss.raw), N.ptr(ss.raw_off), N.ptr(ss.range), N.ptr(ss.digitisation), N.ptr(ss.offset),
                                            N.ptr(n_ev), N.ptr(off), N.ptr(ev), cap, N.ptr(total), N.ptr(status)), ev
    ev = N.call_with_room(call, _cap(ss, event_cap), total, fixed=event_cap is not None)
    return off, ev[:int(total[0])], status[:n]


def signal_align_host(ss, event_cap=None):
    """gbx_abea_signal_align_host -> dict(event_off, events, scale, shift, status, pairs, n_pairs); read r's pairs are
    pairs[2 * event_off[r] : 2 * event_off[r] + n_pairs[r]]."""
    n = ss.n_reads
    off, status, n_pairs = np.zeros(n + 1, np.int64), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    scale, shift = np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.float32)
    total = np.zeros(1, np.int64)

    def call(cap):
        ev, out = np.zeros(max(cap, 1), dtype=EVENT_DTYPE), np.zeros(2 * max(cap, 1), dtype=PAIR_DTYPE)
        return N.lib().gbx_abea_signal_align_host(n, N.ptr(ss.raw), N.ptr(ss.raw_off), N.ptr(ss.range), N.ptr(ss.digitisation), N.ptr(ss.offset),
                                                  N.ptr(ss.seq_off), N.ptr(ss.seq_len), N.ptr(ss.seq_arena), ss.seq_arena.size, N.ptr(ss.model),
                                                  N.ptr(off), N.ptr(ev), cap, N.ptr(total), N.ptr(scale), N.ptr(shift), N.ptr(status),
                                                  N.ptr(out), N.ptr(n_pairs)), (ev, out)
    ev, out = N.call_with_room(call, _cap(ss, event_cap), total, fixed=event_cap is not None)
    t = int(total[0])
    return dict(event_off=off, events=ev[:t], scale=scale[:n], shift=shift[:n], status=status[:n], pairs=out[:2 * max(t, 1)], n_pairs=n_pairs[:n])


class DeviceAbeaSignalSet:
    """An AbeaSignalSet resident in HBM.  run(): count pass, the total comes to the host (the event arrays are sized by it),
    fill pass, scalings.  align_set() hands the result to the existing align path as a DeviceAbeaReadSet."""

    def __init__(self, ss, device):
        import torch
        self.torch, self.device, self.ss = torch, device, ss
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        n = ss.n_reads
        self.n_reads = n
        self.raw = t(np.concatenate([ss.raw, np.zeros(8, np.int16)]))
        self.raw_off, self.range, self.digitisation, self.offset = t(ss.raw_off), t(ss.range), t(ss.digitisation), t(ss.offset)
        self.seq_off, self.seq_len, self.model = t(ss.seq_off), t(ss.seq_len), t(ss.model.view(np.uint8))
        self.seq_arena = t(np.concatenate([ss.seq_arena, np.zeros(16, np.uint8)]))
        z = lambda dt, k=0: torch.zeros(max(n, 1) + k, dtype=dt, device=device)
        self.n_events, self.event_off, self.status = z(torch.int64), z(torch.int64, 1), z(torch.int32)
        self.scale, self.shift = z(torch.float32), z(torch.float32)
        self.events = self.event_mean = None
        self.n_events_total = 0

    def _events(self, pass_, stream):
        ev = self.events.data_ptr() if self.events is not None else None
        em = self.event_mean.data_ptr() if self.event_mean is not None else None
        N.check(N.lib().gbx_abea_events_device(pass_, self.n_reads, self.raw.data_ptr(), self.raw_off.data_ptr(), self.range.data_ptr(),
                                               self.digitisation.data_ptr(), self.offset.data_ptr(), self.n_events.data_ptr(),
                                               self.event_off.data_ptr(), ev, em, self.n_events_total, self.status.data_ptr(), stream))

    def count(self, stream=None):
        self._events(PASS_COUNT, stream)

    def size_outputs(self):
        """after count(): synchronises, brings the total over and allocates the event arrays"""
        torch = self.torch
        self.n_events_total = int(self.event_off[self.n_reads].item()) if self.n_reads else 0
        self.events = torch.zeros((max(self.n_events_total, 1), 24), dtype=torch.uint8, device=self.device)
        self.event_mean = torch.zeros(self.n_events_total + 4, dtype=torch.float32, device=self.device)

    def fill(self, stream=None):
        self._events(PASS_FILL, stream)

    def scalings(self, stream=None):
        N.check(N.lib().gbx_abea_scalings_device(self.n_reads, self.seq_off.data_ptr(), self.seq_len.data_ptr(), self.seq_arena.data_ptr(),
                                                 self.event_off.data_ptr(), self.event_mean.data_ptr(), self.model.data_ptr(),
                                                 self.scale.data_ptr(), self.shift.data_ptr(), stream))

    def run(self, stream=None):
        self.count(stream)
        self.size_outputs()
        self.fill(stream)
        self.scalings(stream)

    def results(self):
        """(event_off, events, scale, shift, status) on the host"""
        n = self.n_reads
        ev = self.events.cpu().numpy().reshape(-1).view(EVENT_DTYPE)[:self.n_events_total]
        return (self.event_off[:n + 1].cpu().numpy(), ev, self.scale[:n].cpu().numpy(), self.shift[:n].cpu().numpy(), self.status[:n].cpu().numpy())

    def align_set(self):
        """(DeviceAbeaReadSet of the reads that have events, their indices): the device arrays go over as they are - reads
        without events take no room in the event array, so the kept reads' absolute offsets still delimit their events."""
        torch = self.torch
        n = self.n_reads
        off = self.event_off[:n + 1].cpu().numpy()
        keep = np.flatnonzero(np.diff(off) > 0)
        kt = torch.from_numpy(keep).to(self.device)
        eoff = np.concatenate([off[keep], off[n:n + 1]]).astype(np.int64)
        d = dict(seq_off=self.seq_off[kt].contiguous(), seq_len=self.seq_len[kt].contiguous(), seq_arena=self.seq_arena,
                 event_off=torch.from_numpy(eoff).to(self.device), event_mean=self.event_mean, scale=self.scale[kt].contiguous(),
                 shift=self.shift[kt].contiguous(), model=self.model)
        return DeviceAbeaReadSet.from_tensors(d, self.device), keep
