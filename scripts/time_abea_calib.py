#!/usr/bin/env python3
"""Times abea's calibration and event-alignment record on one device beside align() on the same reads, and call-methylation
from raw signal in one call beside the composition of entries it replaces, all in one run; the site planner and the job order on
the device beside the host planner and gbx_abea_meth_plan_host on the same record.  Prints one JSON line and writes
profiles/abea_calib_time_<preset>.json.

  python scripts/time_abea_calib.py --preset small|large [--reps N] [--no-write] [--parent-lib build_tmp/libgbx_parent.so]
  python scripts/time_abea_calib.py --preset small|large --one-call-only          (the one call alone, of the library GBX_LIB names)

--parent-lib: a libgbx.so built from the parent commit.  The one call is then timed in fresh processes, the parent's library and
this one alternately (parent, this, parent, this), each with its own warm-up, and both sets of times are recorded.

'large' is the 10 000 reads of abea large (seed 5001) as raw signal with generated CIGARs.  One warm-up, then the median of --reps.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PRESETS = {"small": (256, 5001), "large": (10000, 5001)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", choices=sorted(PRESETS), default="small")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--one-call-only", action="store_true")
    ap.add_argument("--parent-lib")
    a = ap.parse_args()
    import torch
    from genomicsbench_amd import _native as N
    from genomicsbench_amd import abea_calib as AC
    from genomicsbench_amd import abea_meth as AM
    from genomicsbench_amd import abea_signal as AS
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

    if a.one_call_only:
        first = AC.call_methylation_host(ss, cg)
        n_sites = len(first["sites"])
        call_ms, call_all = timed(lambda: AC.call_methylation_host(ss, cg, site_cap=n_sites))
        print(json.dumps(dict(lib=N.LIB_PATH, preset=a.preset, n_sites=n_sites, one_call_ms=call_ms, one_call_ms_all=call_all,
                              scores_crc=int(np.bitwise_xor.reduce(first["scores"].reshape(-1).view(np.uint32))))))
        return 0

    # the stages on the device, on the same reads
    d = AS.DeviceAbeaSignalSet(ss, dev)
    d.run(stream)
    drs, keep = d.align_set()
    align_ms, align_all = timed(lambda: drs.run(stream))
    cal = AC.DeviceAbeaCalib(d, drs, keep, cg["cigar_off"], cg["cigar"], cg["pos"], cg["rc"])
    calib_ms, calib_all = timed(lambda: cal.launch(stream))
    cal.run(stream)
    count_ms, count_all = timed(lambda: cal.record_count(stream))
    cal.record_size()
    fill_ms, fill_all = timed(lambda: cal.record_fill(stream))
    torch.cuda.synchronize()
    c = cal.results()
    rec_off, rec = cal.record_results()
    # the site planner and the job order: on the device where the record lies, and on the host from its copy
    flank_len = int(np.diff(d.event_off[:n_reads + 1].cpu().numpy()).max()) + 1
    sd = AM.DeviceAbeaMethSites(cal, cg["ref_off"], cg["ref_len"], cg["ref_arena"])
    pcount_ms, pcount_all = timed(lambda: sd.count(stream))
    sd.size()
    pfill_ms, pfill_all = timed(lambda: sd.fill(stream))
    order_ms, order_all = timed(lambda: sd.order(flank_len, stream))              # with its workspace and the 48 bytes it brings back
    host_sites = []
    hplan_ms, hplan_all = timed(lambda: host_sites.append(AM.sites_host(cg["ref_off"], cg["ref_len"], cg["ref_arena"], cg["pos"], cg["rc"], rec_off, rec)))
    h_sites, h_jobs, h_arena = host_sites[-1]
    js = AM.AbeaMethJobSet(h_jobs, h_arena, d.event_off[:n_reads + 1].cpu().numpy(), np.zeros(0, np.float32), c["scale"], c["shift"], c["var"], c["log_var"],
                           c["events_per_base"], cg["cpg_model"])
    plans = []
    hord_ms, hord_all = timed(lambda: plans.append(js.plan()))
    g_sites, g_jobs, g_arena = sd.results()
    planner_same = bool(np.array_equal(g_sites, h_sites) and np.array_equal(g_jobs, h_jobs) and np.array_equal(g_arena, h_arena) and
                        np.array_equal(sd.order_.cpu().numpy()[:len(h_jobs)], plans[-1]["order"][:len(h_jobs)]) and
                        np.array_equal(sd.class_off, plans[-1]["class_off"]))
    longest = int(np.argmax(ss.seq_len))
    one = AS.DeviceAbeaSignalSet(ss.take([longest]), dev)
    one.run(stream)
    drs1, keep1 = one.align_set()
    drs1.run(stream)
    k0, k1 = int(cg["cigar_off"][longest]), int(cg["cigar_off"][longest + 1])
    cal1 = AC.DeviceAbeaCalib(one, drs1, keep1, [0, k1 - k0], cg["cigar"][k0:k1], cg["pos"][longest:longest + 1], cg["rc"][longest:longest + 1])
    calib1_ms, _ = timed(lambda: cal1.launch(stream))

    # the one call, and the composition it replaces fed the same calibration
    t = time.perf_counter()
    first = AC.call_methylation_host(ss, cg)
    first_ms = (time.perf_counter() - t) * 1e3
    n_sites = len(first["sites"])
    call_ms, call_all = timed(lambda: AC.call_methylation_host(ss, cg, site_cap=n_sites))
    parts = {}

    def composition():
        t0 = time.perf_counter()
        r = AS.signal_align_host(ss)
        t1 = time.perf_counter()
        sites, jobs, arena = AM.sites_host(cg["ref_off"], cg["ref_len"], cg["ref_arena"], cg["pos"], cg["rc"], rec_off, rec)
        t2 = time.perf_counter()
        scores = np.zeros(max(len(jobs), 1), np.float32)
        cpg, ev = np.ascontiguousarray(cg["cpg_model"]), r["events"] if len(r["events"]) else np.zeros(1, r["events"].dtype)
        N.check(N.lib().gbx_abea_meth_score_host(len(jobs), N.ptr(jobs), N.ptr(arena), arena.size, n_reads, N.ptr(r["event_off"]), N.ptr(ev),
                                                 N.ptr(c["scale"]), N.ptr(c["shift"]), N.ptr(c["var"]), N.ptr(c["log_var"]),
                                                 N.ptr(c["events_per_base"]), N.ptr(cpg), N.ptr(scores)))
        t3 = time.perf_counter()
        parts.update(signal_align_host_ms=round((t1 - t0) * 1e3, 3), planner_ms=round((t2 - t1) * 1e3, 3), score_host_ms=round((t3 - t2) * 1e3, 3))
        parts["scores"], parts["jobs"], parts["arena"], parts["events"], parts["pairs"] = scores, len(jobs), arena.size, len(r["events"]), int(r["n_pairs"].sum())

    comp_ms, comp_all = timed(composition)
    same = bool(np.array_equal(first["scores"].reshape(-1).view(np.uint32), parts["scores"][:2 * n_sites].view(np.uint32))) and 2 * n_sites == parts["jobs"]
    same = same and bool(np.array_equal(first["flags"], c["flags"]))
    n_cig = len(cg["cigar"])
    small = n_reads * 64                              # the per-read tables that go up; computed from array sizes, not measured
    moved = dict(
        # the reference segments with their offsets and lengths go up; no job and no string does
        one_call_up=int(ss.raw.nbytes + ss.seq_arena.nbytes + 4 * n_cig + 13 * n_reads + cg["ref_arena"].nbytes + 12 * n_reads + small),
        # event counts 8 and status 4 per read; calibration 36 per read (scale, shift, var, var64, events_per_base, n_m_state, flags);
        # the record's total 8, the planner's two totals 16 and its strand flags, the order's 48, the site table and the scores
        one_call_down=int(12 * n_reads + 36 * n_reads + 8 + 16 + n_reads + 48 + 32 * n_sites + 4 * parts["jobs"]),
        # what the one call moved while the planner and the plan ran on the host (the parent commit)
        one_call_host_planner_up=int(ss.raw.nbytes + ss.seq_arena.nbytes + 4 * n_cig + 13 * n_reads + 40 * parts["jobs"] + parts["arena"] + small),
        one_call_host_planner_down=int(12 * n_reads + 36 * n_reads + 8 * (n_reads + 1) + 8 * len(rec) + 4 * parts["jobs"]),
        composition_up=int(ss.raw.nbytes + ss.seq_arena.nbytes + 4 * parts["events"] + 40 * parts["jobs"] + parts["arena"] + small),
        composition_down=int(12 * n_reads + 8 * n_reads + 24 * parts["events"] + 8 * parts["pairs"] + 4 * parts["jobs"]))
    ab = None
    if a.parent_lib:                                  # fresh processes, the two libraries alternately
        ab = dict(order="parent, this, parent, this", parent_ms_all=[], this_ms_all=[], parent_lib=os.path.basename(a.parent_lib))
        crc = set()
        for lib in (a.parent_lib, None, a.parent_lib, None):
            env = dict(os.environ)
            if lib:
                env["GBX_LIB"] = os.path.abspath(lib)
            else:
                env.pop("GBX_LIB", None)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--preset", a.preset, "--reps", str(a.reps), "--one-call-only"], env=env,
                               capture_output=True, text=True, check=True)
            o = json.loads(r.stdout.strip().splitlines()[-1])
            ab["parent_ms_all" if lib else "this_ms_all"] += o["one_call_ms_all"]
            crc.add((o["n_sites"], o["scores_crc"]))
        ab.update(parent_ms=round(float(np.median(ab["parent_ms_all"])), 3), this_ms=round(float(np.median(ab["this_ms_all"])), 3),
                  parent_spread_ms=round(max(ab["parent_ms_all"]) - min(ab["parent_ms_all"]), 3), same_scores=len(crc) == 1)
    res = dict(kernel="abea_calib", preset=a.preset, n_reads=n_reads, seed=seed, n_events=int(d.n_events_total), n_kmers=int((ss.seq_len - 5).sum()),
               longest_read=int(ss.seq_len.max()), n_cigar=n_cig, n_record=int(len(rec)), n_sites=n_sites, flagged=int((c["flags"] != 0).sum()),
               device=torch.cuda.get_device_name(0), reps=a.reps, align_ms=align_ms, align_ms_all=align_all, calib_ms=calib_ms, calib_ms_all=calib_all,
               calib_longest_read_alone_ms=calib1_ms, record_count_ms=count_ms, record_count_ms_all=count_all, record_fill_ms=fill_ms,
               record_fill_ms_all=fill_all, calib_plus_record_ms=round(calib_ms + count_ms + fill_ms, 3), one_call_first_ms=round(first_ms, 3),
               one_call_ms=call_ms, one_call_ms_all=call_all, composition_ms=comp_ms, composition_ms_all=comp_all,
               composition_parts_ms={k: v for k, v in parts.items() if k.endswith("_ms")},
               planner_count_ms=pcount_ms, planner_count_ms_all=pcount_all, planner_fill_ms=pfill_ms, planner_fill_ms_all=pfill_all, order_ms=order_ms,
               order_ms_all=order_all, planner_plus_order_ms=round(pcount_ms + pfill_ms + order_ms, 3), host_planner_ms=hplan_ms,
               host_planner_ms_all=hplan_all, host_plan_ms=hord_ms, host_plan_ms_all=hord_all, host_planner_plus_plan_ms=round(hplan_ms + hord_ms, 3),
               planner_and_order_equal_host=planner_same, n_jobs=int(len(h_jobs)), string_bytes=int(h_arena.size), one_call_ab=ab, bytes_moved=moved,
               bytes_moved_source="computed from the sizes of the arrays each path copies", one_call_equals_composition=same)
    line = json.dumps(res)
    print(line)
    if not a.no_write:
        with open(os.path.join(ROOT, "profiles", "abea_calib_time_%s.json" % a.preset), "w") as f:
            f.write(line + "\n")
    return 0 if same and planner_same and (ab is None or ab["same_scores"]) else 1


if __name__ == "__main__":
    sys.exit(main())
