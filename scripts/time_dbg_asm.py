"""Times the dbg assembly stage on one preset: gbx_dbg_assemble_device (median of --reps) beside the build step
(gbx_dbg_build_device) in the same run and their ratio, the host entry, and per k round the windows built and the time of
the build, the cycle check, the start list and the path search.  The rounds' times come from the library's per-kernel
profile of calls cut short at each round (k_last = the round's k - 1): a round is the difference of two such calls.  A
seeded sample of windows is held against the restatement (tests/dbg_asm_ref.py).  Prints one JSON line and writes it to
profiles/dbg_asm_time_<preset>.json, or, with the preset's contig length overridden, to
profiles/dbg_asm_time_<preset>_len<N>.json (the record says so too).
    python scripts/time_dbg_asm.py --preset large [--contig-len N] [--reps 3] [--sample 6]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
STAGES = {"build": ("dbg_init", "dbg_insert", "dbg_finish"), "cycle": ("dbg_asm_cycle",), "starts": ("dbg_asm_starts",), "search": ("dbg_asm_search",)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="large")
    ap.add_argument("--contig-len", type=int, default=0, help="override the preset's contig length")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sample", type=int, default=6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import dbg_asm_ref as AR
    from genomicsbench_amd import _native as N, dbg as D, dbg_asm as A, pileup as P
    from genomicsbench_amd.datagen import DBG_PRESETS, gen_dbg_reads
    pr = dict(DBG_PRESETS[a.preset])
    if a.contig_len:
        pr["contig_len"] = a.contig_len
    c, recs, fa = gen_dbg_reads(pr["contig_len"], pr["coverage"], pr["seed"])
    d = tempfile.mkdtemp()
    bam, fasta = os.path.join(d, "d.bam"), os.path.join(d, "d.fa")
    P.write_bam(bam, c, recs)
    with open(fasta, "wb") as f:
        f.write(fa)
    del recs
    rs, (ctg, beg, end), _ = D.read_bam(bam, c[0][0])
    wins = D.make_windows(rs, beg, end, D.read_fasta(fasta)[ctg])
    print("ingest done: %d reads, %d windows" % (rs.n_reads, wins.n_win), flush=True)
    s = torch.cuda.current_stream()

    def timed(call, reps):
        ms = []
        for _ in range(reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            call()
            e1.record(s)
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms[1:])), [round(x, 3) for x in ms[1:]]

    dd = D.DeviceDbg(rs, wins, "cuda:0")
    build_ms, build_all = timed(lambda: dd.build(s.cuda_stream), a.reps)
    del dd
    caps = (1 << 20, 1 << 20, 1 << 26)
    da = A.DeviceAsm(rs, wins, "cuda:0", caps=caps)
    asm_ms, asm_all = timed(lambda: N.check(da.assemble(s.cuda_stream)), a.reps)
    res = da.results()
    out = dict(preset=a.preset, contig_len=pr["contig_len"], contig_len_overridden=bool(a.contig_len), reads=rs.n_reads, windows=wins.n_win, build_ms=round(build_ms, 3), build_ms_all=build_all,
               assemble_ms=round(asm_ms, 3), assemble_ms_all=asm_all, assemble_over_build=round(asm_ms / build_ms, 3),
               workspace_bytes=int(da.work_bytes), starts=len(res.starts), paths=len(res.paths), path_nodes=len(res.path_nodes),
               gave_up=int(res.wins["n_gave_up"].sum()), step_capped=int(res.wins["n_steps"].sum()), cyclic_at_the_end=int(res.wins["cyclic"].sum()))
    # per round: calls cut short behind round r
    p, ap0, rounds, before = D.make_params(), A.make_asm_params(), [], {f: 0.0 for f in STAGES}
    n_rounds = int(res.wins["n_builds"].max())
    for r in range(1, n_rounds + 1):
        k = p.k + ap0.k_step * (r - 1)
        cut = A.DeviceAsm(rs, wins, "cuda:0", asm_params=A.make_asm_params(k_last=k - 1), caps=caps)
        cut.assemble(s.cuda_stream)                       # warm
        N.profile_begin()
        cut.assemble(s.cuda_stream)
        prof = N.profile_end()
        del cut
        now = {f: sum(prof.get(n, (0.0, 0))[0] for n in names) for f, names in STAGES.items()}
        rounds.append(dict(k=k, windows=int((res.wins["n_builds"] >= r).sum()), **{f + "_ms": round(now[f] - before[f], 3) for f in STAGES}))
        before = now
    out["rounds"] = rounds
    A.assemble_host(rs, wins, caps=caps)
    t = time.time()
    hres = A.assemble_host(rs, wins, caps=caps)
    out["host_ms"] = round((time.time() - t) * 1e3, 3)
    assert hres.wins.tobytes() == res.wins.tobytes() and hres.paths.tobytes() == res.paths.tobytes(), "host entry differs from the device entry"
    rng = np.random.default_rng(7)
    sample = sorted(rng.choice(wins.n_win, size=min(a.sample, wins.n_win), replace=False).tolist())
    ok = 0
    for w in sample:
        want = AR.window(wins.window_ref(w), int(wins.ref_pos[w]), [rs.read(r) for r in range(wins.read_lo[w], wins.read_hi[w])])
        got = res.window(w)
        ok += all(got[f] == want[f] for f in ("k", "n_builds", "cyclic", "n_paths", "n_path_nodes", "n_gave_up", "n_steps", "stats")) and \
            [(g["node"], g["edge"], g["status"], g["paths"]) for g in got["starts"]] == [(h["node"], h["edge"], h["status"], h["paths"]) for h in want["starts"]]
    out["sample_windows"] = sample
    out["sample_verified"] = "%d/%d" % (ok, len(sample))
    line = json.dumps(out)
    print(line)
    name = "dbg_asm_time_%s.json" % a.preset if not a.contig_len else "dbg_asm_time_%s_len%d.json" % (a.preset, a.contig_len)
    with open(a.out or os.path.join(ROOT, "profiles", name), "w") as f:
        f.write(line + "\n")
    return 0 if ok == len(sample) else 1


if __name__ == "__main__":
    sys.exit(main())
