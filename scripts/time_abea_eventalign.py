#!/usr/bin/env python3
"""Times abea's eventalign step on one device beside align() and the calibration on the same reads, the C restatement of the
step on 16 threads, the host entry and eventalign from raw signal in one call, all in one run.  Prints one JSON line and writes
profiles/abea_eventalign_time_<preset>.json.

  python scripts/time_abea_eventalign.py --preset small|large [--reps N] [--no-write]

'large' is the 10 000 reads of abea large (seed 5001) as raw signal with generated CIGARs.  One warm-up, then the median of --reps.
The fill and the traceback run in one kernel and are not timed apart; the cells and the traceback steps are counted instead.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PRESETS = {"small": (256, 5001), "large": (10000, 5001)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", choices=sorted(PRESETS), default="small")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    import torch
    import abea_eventalign_ref as R
    from genomicsbench_amd import abea_calib as AC
    from genomicsbench_amd import abea_eventalign as EA
    from genomicsbench_amd import abea_signal as AS
    from genomicsbench_amd.abea import EVENT_DTYPE
    from genomicsbench_amd.datagen import gen_abea_cigars, gen_abea_raw

    n_reads, seed = PRESETS[a.preset]
    ss = gen_abea_raw(n_reads, seed)
    cg = gen_abea_cigars(ss, seed)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream

    def timed(fn, reps=a.reps):
        out = []
        for k in range(reps + 1):                     # the first run is the warm-up
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t) * 1e3)
        return round(float(np.median(out[1:])), 3), [round(x, 3) for x in out[1:]]

    def chain(sig, cig_off, cig, pos, rc):
        d = AS.DeviceAbeaSignalSet(sig, dev)
        d.run(stream)
        drs, keep = d.align_set()
        drs.run(stream)
        cal = AC.DeviceAbeaCalib(d, drs, keep, cig_off, cig, pos, rc)
        cal.run(stream)
        cal.record_count(stream)
        return d, drs, cal

    # the stages on the device, on the same reads
    d, drs, cal = chain(ss, cg["cigar_off"], cg["cigar"], cg["pos"], cg["rc"])
    align_ms, align_all = timed(lambda: drs.run(stream))
    calib_ms, calib_all = timed(lambda: cal.launch(stream))
    cal.run(stream)
    count_ms, count_all = timed(lambda: cal.record_count(stream))
    ea = EA.DeviceAbeaEventalign(cal, cg["ref_off"], cg["ref_len"], cg["ref_arena"], counts=True)
    ea_ms, ea_all = timed(lambda: ea.run(stream))
    got = ea.results()
    counts = ea.counts.cpu().numpy()[:n_reads]
    # the longest read alone: per read the step is a serial chain of segments
    longest = int(np.argmax(np.diff(d.event_off[:n_reads + 1].cpu().numpy())))
    k0, k1 = int(cg["cigar_off"][longest]), int(cg["cigar_off"][longest + 1])
    r0 = int(cg["ref_off"][longest])
    _, _, cal1 = chain(ss.take([longest]), [0, k1 - k0], cg["cigar"][k0:k1], cg["pos"][longest:longest + 1], cg["rc"][longest:longest + 1])
    ea1 = EA.DeviceAbeaEventalign(cal1, [0], cg["ref_len"][longest:longest + 1], cg["ref_arena"][r0:r0 + int(cg["ref_len"][longest])])
    ea1_ms, _ = timed(lambda: ea1.run(stream))

    # the C restatement on 16 threads, on the calibration the device computed
    c = cal.results()
    event_off = d.event_off[:n_reads + 1].cpu().numpy()
    events = d.events.cpu().numpy().view(EVENT_DTYPE).reshape(-1)[:int(event_off[-1])]
    means = np.ascontiguousarray(events["mean"])
    t = time.perf_counter()
    want = R.run(ss.seq_off, ss.seq_len, event_off, means, ss.model, c, cg, threads=16)
    cpu_ms = (time.perf_counter() - t) * 1e3
    same = bool(np.array_equal(got["n_rec"], want["n_rec"]) and np.array_equal(got["status"], want["status"]) and np.array_equal(counts, want["counts"]))
    for r in range(n_reads):
        same = same and bool(np.array_equal(R.read_records(got, event_off, r), R.read_records(want, event_off, r)))

    # the host entry (the calibration's results and the events go up) and the one call from raw signal
    host_ms, host_all = timed(lambda: EA.eventalign_host(ss.seq_off, ss.seq_len, event_off, events, ss.model, c, cg))
    first = EA.eventalign_from_signal_host(ss, cg)
    call_ms, call_all = timed(lambda: EA.eventalign_from_signal_host(ss, cg, event_cap=len(first["events"])))
    same = same and bool(np.array_equal(first["n_rec"], want["n_rec"]) and np.array_equal(first["rec"], got["rec"]))
    res = dict(kernel="abea_eventalign", preset=a.preset, n_reads=n_reads, seed=seed, n_events=int(event_off[-1]), n_kmers=int((ss.seq_len - 5).sum()),
               longest_read=int(ss.seq_len.max()), longest_read_events=int(np.diff(event_off).max()), n_cigar=len(cg["cigar"]), flagged=int((c["flags"] != 0).sum()),
               records=int(want["n_rec"].sum()), segments=int(counts[:, 0].sum()), cells=int(counts[:, 1].sum()), traceback_steps=int(counts[:, 2].sum()),
               segments_longest_read=int(counts[longest, 0]), status_nonzero=int((want["status"] != 0).sum()), rows_cap=EA.ROWS_CAP,
               workspace_bytes=ea.work_bytes, device=torch.cuda.get_device_name(0), reps=a.reps, eventalign_ms=ea_ms, eventalign_ms_all=ea_all,
               eventalign_longest_read_alone_ms=ea1_ms, gcells_per_s=round(float(counts[:, 1].sum()) / ea_ms / 1e6, 3), align_ms=align_ms, align_ms_all=align_all,
               calib_ms=calib_ms, calib_ms_all=calib_all, record_count_ms=count_ms, record_count_ms_all=count_all,
               restatement_16_threads_ms=round(cpu_ms, 3), host_entry_ms=host_ms, host_entry_ms_all=host_all, one_call_ms=call_ms, one_call_ms_all=call_all,
               fill_and_traceback="one kernel, not timed apart", device_equals_restatement=same)
    line = json.dumps(res)
    print(line)
    if not a.no_write:
        with open(os.path.join(ROOT, "profiles", "abea_eventalign_time_%s.json" % a.preset), "w") as f:
            f.write(line + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
