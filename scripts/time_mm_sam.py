#!/usr/bin/env python3
"""Times the mm sam stage (genomicsbench_amd.mm_sam) on the input of scripts/time_mm_seed.py and writes one JSON line to
profiles/mm_sam_time.json (--preset large) or profiles/mm_sam_time_small.json (--preset small):

  align        gbx_mm_align_device, re-measured in this run (device events)
  paf_cigar    gbx_mm_paf_cigar_device: the text with cg:Z:, the stage this one stands beside
  sets         for PAF + cs, SAM, SAM + cs + MD + eqx: gbx_mm_sam_device on the same stream, best of the repeats after a warm-up;
               its text bytes per second; the download of its own text into pinned memory; the ratios to both yardsticks
  validated    the first reads' SAM lines through tests/mm_sam_ref.py's validator

--preset large = --genome 67108864 --reads 4000 --read-len 10000; small = --genome 4194304 --reads 400.  Needs a GPU: no fallback.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SETS = (("paf_cs", dict(cs=1)), ("sam", dict(format=1)), ("sam_cs_md_eqx", dict(format=1, cs=1, md=1, eqx=1)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--preset", choices=["large", "small"])
    ap.add_argument("--genome", type=int, default=1 << 22)
    ap.add_argument("--reads", type=int, default=400)
    ap.add_argument("--read-len", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--validate-reads", type=int, default=20, help="the reads whose SAM lines go through the validator")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.preset == "large":
        a.genome, a.reads, a.read_len = 1 << 26, 4000, 10000
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "mm_sam_time.json" if a.preset == "large" else "mm_sam_time_small.json")
    import torch
    from genomicsbench_amd import _native as N
    from genomicsbench_amd import mm_map as MM
    from genomicsbench_amd import mm_sam as MSAM
    from genomicsbench_amd import mm_seed as MS
    from time_mm_seed import make_inputs
    import mm_sam_ref as SR
    if not torch.cuda.is_available() or N.device_count() < 1:
        sys.exit("time_mm_sam.py needs a GPU")
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    refs, reads = make_inputs(a.genome, a.reads, a.read_len, a.seed)
    quals = [bytes(33 + (7 * i) % 40 for i in range(len(r))) for r in reads]
    timer = N.StreamTimer()

    def timed(fn, reps):
        fn()                                                         # the warm-up
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            timer.start(s)
            fn()
            timer.stop(s)
            torch.cuda.synchronize()
            ms.append(timer.elapsed_ms())
        return min(ms), [round(x, 3) for x in ms]

    ix = MS.DeviceMmIndex(MS.make_params(), refs, dev, s, mini_cap=max(a.genome // 4, 1024))
    sd = MS.DeviceMmSeeder(ix, reads, mini_cap=max(sum(len(r) for r in reads) // 4, 1024), anchor_cap=1024)
    sd.run(s)
    n_mini, n_anchor = sd.counts()
    sd = MS.DeviceMmSeeder(ix, reads, mini_cap=n_mini, anchor_cap=max(n_anchor, 1))
    mp = MM.DeviceMmMapper(sd)
    mp.run(s)
    n_chain, n_reg, _ = mp.counts()
    assert mp.fits()
    # sized by runs that report the needs: the jobs' room, the words, the text
    mp = MM.DeviceMmMapper(sd, chain_cap=max(n_chain, 1), reg_cap=max(n_reg, 1), text_cap=1, align=True)
    al = mp.aligner
    al.caps = (1, 16, 1)
    mp.run(s)
    z_need = al.counts()[2]
    al.caps, al.sized_for = (1, z_need, 1), None
    al.run(s)
    n_words = al.counts()[1]
    al.caps, al.sized_for = (max(n_words, 1), z_need, 1), None
    al.run(s)
    n_text = al.counts()[3]
    al.caps, al.sized_for = (max(n_words, 1), z_need, max(n_text, 1)), None
    al.run(s)
    assert al.fits()
    align_ms, align_all = timed(lambda: al.run_align(s), a.repeats)
    paf_ms, paf_all = timed(lambda: al.run_paf(s), a.repeats)
    sets, validated = {}, 0
    for name, o in SETS:
        st = MSAM.DeviceMmSam(al, MSAM.make_params(**o), quals=quals, text_cap=1)
        st.run(s)
        need = st.counts()[2]
        st = MSAM.DeviceMmSam(al, MSAM.make_params(**o), quals=quals, text_cap=need)
        st.run(s)
        assert st.fits() and st.counts()[2] == need
        ms, ms_all = timed(lambda: st.run(s), a.repeats)
        pinned = torch.empty(need, dtype=torch.uint8).pin_memory()
        dl_ms, dl_all = timed(lambda: pinned.copy_(st.lines[:need], non_blocking=True), a.repeats)
        lines_n, silent, _ = st.counts()
        if o.get("format"):
            k = min(a.validate_reads, a.reads)
            lo = st.results()["line_off"]
            head = pinned[:int(lo[k])].numpy().tobytes().decode()
            validated = SR.validate(head, [("read%d" % i, reads[i].decode()) for i in range(k)], [("ref%d" % i, r.decode()) for i, r in enumerate(refs)],
                                    [int(v) for v in lo[:k + 1]])
            assert validated > 0
        sets[name] = dict(options=o, ms=round(ms, 3), ms_all=ms_all, bytes=need, lines=lines_n, silent_regions=silent, gbytes_per_s=round(need / (ms * 1e-3) / 1e9, 3),
                          download_ms=round(dl_ms, 3), download_ms_all=dl_all, over_align=round(ms / align_ms, 4), over_download=round(ms / dl_ms, 3),
                          over_paf_cigar=round(ms / paf_ms, 2), validated_records=validated if o.get("format") else None)
    rec = dict(what="the mm sam stage beside the align stage, the PAF-with-CIGAR text and the download of its own text in the same run, one stream; device events, "
                    "a warm-up, best of the repeats", genome_bp=a.genome, reads=a.reads, read_len=a.read_len, seed=a.seed, regions=n_reg, cigar_words=n_words,
               align=dict(ms=round(align_ms, 3), ms_all=align_all), paf_cigar=dict(ms=round(paf_ms, 3), ms_all=paf_all, bytes=n_text), sets=sets,
               device=torch.cuda.get_device_name(0))
    line = json.dumps(rec)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
