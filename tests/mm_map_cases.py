"""Seeded cases for the stage behind the chain scores (tests/mm_map_ref.py is the restatement).  The generators assert their own
coverage, so a case that stops exercising its path fails here and not silently."""
import functools
import random

import numpy as np

import mm_cases as K
import mm_map_ref as MR
import mm_ref as R

FOREST_PARAMS = [(40, 3), (15, 2), (15, 1)]                   # (min_chain_score, min_cnt)
FOREST_SIZES = (0, 1, 2, 63, 64, 65, 257, 5000, 300, 40, 7, 0, 129)
MAP_PARAMS = dict(k=15, w=10, is_hpc=0, mid_occ=20)


def forest(rng, n):
    """One read's (f, p, v, ax, ay, qlen) built directly: a forest whose parents lie at most six anchors back, scores that rise
    and fall along a path, v the running peak - and on a few paths a v above every f, so that the peak search runs off the root."""
    f, p, v = [], [], []
    for i in range(n):
        pi = -1 if i == 0 or rng.random() < 0.12 else rng.randrange(max(0, i - 6), i)
        if pi < 0:
            fi = rng.randrange(10, 25)
            vi = fi
        else:
            fi = max(1, f[pi] + (rng.randrange(-8, 20) if rng.random() > 0.05 else 45))      # a jump: a short branch that scores
            vi = max(v[pi], fi)
        f.append(fi), p.append(pi), v.append(vi)
    children = set(p)
    leaves = [i for i in range(n) if i not in children]
    for i in rng.sample(leaves, min(len(leaves), 2 + n // 200)) if n >= 3 else []:
        top = max(f) + 3
        j = i
        while j >= 0:
            v[j] = max(v[j], top)
            j = p[j]
    ax, ay = [], []
    pos = [0, 0, 0]
    for i in range(n):
        blk = 0 if i < n // 2 else 1 if i < 3 * n // 4 else 2       # rid 0 forward, rid 1 forward, rid 0 reverse: x ascending
        pos[blk] += rng.choice([0, 0, 3, 9, 15])
        ax.append((blk == 2) << 63 | (blk == 1) << 32 | pos[blk])
        span = rng.choice([15, 15, 15, 12, 20])
        ay.append((rng.random() < 0.1) << 42 | span << 32 | (50 + 7 * i + rng.randrange(6)))
    return f, p, v, ax, ay, 50 + 7 * n + 100


@functools.lru_cache(maxsize=None)
def forest_batch():
    """-> dict of the flat arrays of one call: reads of every size in FOREST_SIZES"""
    rng = random.Random(31337)
    rs = [forest(rng, n) for n in FOREST_SIZES]
    off = np.zeros(len(rs) + 1, np.int64)
    np.cumsum([len(r[0]) for r in rs], out=off[1:])
    cat = lambda k, dt: np.array([x for r in rs for x in r[k]], dtype=dt)
    qlen = np.array([r[5] for r in rs], np.int64)
    seq_off = np.zeros(len(rs) + 1, np.int64)
    np.cumsum(qlen, out=seq_off[1:])
    return dict(off=off, f=cat(0, np.int32), p=cat(1, np.int32), v=cat(2, np.int32), ax=cat(3, np.uint64), ay=cat(4, np.uint64), qlen=qlen,
                seq_off=seq_off, rep_len=np.array([rng.choice([0, 0, 35, 300]) for _ in rs], np.int32),
                hash=np.array([rng.getrandbits(32) for _ in rs], np.uint32))


def expected(b, **kw):
    return MR.map_batch(b["off"], b["ax"], b["ay"], b["f"], b["p"], b["v"], b["qlen"], b["rep_len"], b["hash"], **kw)


def same(got, want, b):
    """every output array of a call equal to the restatement's; the chained anchors up to each read's count"""
    for k in ("chain_off", "u", "n_chained", "reg_off"):
        assert np.array_equal(got[k], want[k]), k
    for r in range(len(b["off"]) - 1):
        lo, hi = int(b["off"][r]), int(b["off"][r]) + int(want["n_chained"][r])
        assert np.array_equal(got["cax"][lo:hi], want["cax"][lo:hi]) and np.array_equal(got["cay"][lo:hi], want["cay"][lo:hi]), r
    assert len(got["regs"]) == len(want["regs"]["id"])
    for k in MR.REG_FIELDS:
        assert np.array_equal(got["regs"][k].astype(np.int64), want["regs"][k]), k


@functools.lru_cache(maxsize=None)
def forest_expected(min_sc, min_cnt):
    st = {}
    exp = expected(forest_batch(), min_chain_score=min_sc, min_cnt=min_cnt, stats=st)
    exp["stats"] = st
    return exp


@functools.lru_cache(maxsize=None)
def forest_coverage():
    """The paths the three parameter sets take together, asserted"""
    tot = {}
    for ps in FOREST_PARAMS:
        e = forest_expected(*ps)
        for k, n in e["stats"].items():
            tot[k] = tot.get(k, 0) + n
        g = e["regs"]
        sec = g["parent"] != g["id"]
        tot["secondary"] = tot.get("secondary", 0) + int(sec.sum())
        tot["n_sub"] = tot.get("n_sub", 0) + int((g["n_sub"] > 0).sum())
        tot["mapq_mid"] = tot.get("mapq_mid", 0) + int(((g["mapq"] > 0) & (g["mapq"] < 60)).sum())
        tot["rs_clamped"] = tot.get("rs_clamped", 0) + int((g["rs"] == 0).sum())
    for k in ("dup_peak", "peak_in_walk", "stop_kept", "stop_dropped", "off_root", "no_end", "cut_by_dropped", "secondary", "n_sub", "mapq_mid"):
        assert tot.get(k, 0) > 0, "the forests never take the path `%s`" % k
    s401 = forest_expected(40, 3)["stats"]
    assert s401.get("stop_dropped", 0) and s401.get("stop_kept", 0) and s401.get("dup_peak", 0)
    return tot


@functools.lru_cache(maxsize=None)
def map_case():
    """mm_cases.seed_case() with a third reference sequence that holds a second, slightly changed copy of a segment of the second,
    and three more reads: one across that segment (a secondary), one of two halves from two places (two primaries), one reverse.
    Chained by the chain oracle on the CPU.  -> dict(refs, reads, qnames, tnames, seeds, f, p, v, target, batch, exp)"""
    from oracle import oracle_py as O
    refs, reads, _ = K.seed_case()
    rng = random.Random(2468)
    r0, r1 = refs
    r2 = K.rand_seq(rng, 1500) + K.mutate(rng, r1[2000:2800], 0.01) + K.rand_seq(rng, 1500)
    refs = (r0, r1, r2)
    reads = tuple(reads) + (K.mutate(rng, r1[1980:2820], 0.03), K.mutate(rng, r0[1000:1700], 0.03) + K.mutate(rng, r1[4000:4700], 0.03),
                            K.mutate(rng, K.revcomp(r2[100:1400]), 0.04))
    idx = R.Index(refs, MAP_PARAMS["w"], MAP_PARAMS["k"], False, mid_occ=MAP_PARAMS["mid_occ"])
    seeds = R.seed_batch(idx, reads)
    f, p, target, v = O.chain_oracle(seeds["off"], seeds["ax"], seeds["ay"], seeds["hdr"])
    off = seeds["off"]
    for r in range(len(reads)):                                  # chain's parents are local to the call and point backwards
        loc, pp = np.arange(off[r + 1] - off[r]), p[off[r]:off[r + 1]]
        assert ((pp >= -1) & (pp < loc)).all()
    qnames = ["read%d" % i for i in range(len(reads))]
    tnames = ["ref%d" % i for i in range(len(refs))]
    qlen = np.array([len(r) for r in reads], np.int64)
    seq_off = np.zeros(len(reads) + 1, np.int64)
    np.cumsum(qlen, out=seq_off[1:])
    batch = dict(off=off, ax=seeds["ax"], ay=seeds["ay"], f=f, p=p, v=v, qlen=qlen, seq_off=seq_off, rep_len=seeds["rep_len"],
                 hash=np.array([MR.read_hash(nm, int(ln)) for nm, ln in zip(qnames, qlen)], np.uint32))
    exp = expected(batch)
    g, ro = exp["regs"], exp["reg_off"]
    per_read = np.diff(ro)
    pri = g["parent"] == g["id"]
    assert (g["rev"] == 1).any(), "no reverse-strand region"
    assert (~pri).any(), "no secondary"
    assert any(pri[ro[r]:ro[r + 1]].sum() >= 2 for r in range(len(reads))), "no read with two primaries"
    assert any(seeds["rep_len"][r] > 0 and per_read[r] > 0 for r in range(len(reads))), "no mapped read with rep_len > 0"
    assert (per_read == 0).any() and (per_read > 0).sum() >= 10, "no read without regions"
    assert (g["subsc"][pri] > 0).any() and len(set(g["mapq"][pri].tolist())) >= 2
    text = MR.paf(g, ro, qnames, qlen, tnames, [len(r) for r in refs], seeds["rep_len"])
    return dict(refs=refs, reads=reads, qnames=qnames, tnames=tnames, seeds=seeds, batch=batch, exp=exp, paf=text)


def device_paf(regs, reg_off, qnames, seq_off, rep_len, tnames, tseq_off, reg_cap, text_cap, alns=None, cigar=None):
    """gbx_mm_paf_device - with alns gbx_mm_paf_cigar_device - on host arrays: room for reg_cap regions (and records), what lies behind
    the count filled with 0x5a, the text in front of guard bytes -> dict(text: the bytes below text_cap, n_text, line_off, intact:
    nothing behind text_cap was touched)"""
    import ctypes as C
    import torch
    from genomicsbench_amd import _native as N
    from genomicsbench_amd import mm_align as MA
    from genomicsbench_amd import mm_map as MM
    d = torch.device("cuda:0")
    n, nr = len(reg_off) - 1, len(regs)
    assert nr <= reg_cap

    def t(a, dt, room=0):
        buf = np.full(max(room * np.dtype(dt).itemsize, np.dtype(dt).itemsize, len(a) * np.dtype(dt).itemsize), 0x5a, np.uint8)
        raw = np.ascontiguousarray(a, dtype=dt).view(np.uint8)
        buf[:len(raw)] = raw
        return torch.from_numpy(buf).to(d)
    qn, qo = MM.pack_names(qnames)
    tn, to = MM.pack_names(tnames)
    keep = [t(regs, MM.REG_DTYPE, reg_cap), t(reg_off, np.int64), t([nr], np.int64), t(qn, np.uint8), t(qo, np.int64), t(seq_off, np.int64),
            t(rep_len, np.int32), t(tn, np.uint8), t(to, np.int64), t(tseq_off, np.int64)]
    g, ro, n_regs, qn, qo, so, rep, tn, to_, tso = [x.data_ptr() for x in keep]
    room = 64
    out = torch.full((text_cap + room,), 0x5a, dtype=torch.uint8, device=d)
    lo, nt = torch.full((n + 1,), -7, dtype=torch.int64, device=d), torch.full((1,), -7, dtype=torch.int64, device=d)
    s = torch.cuda.current_stream().cuda_stream
    if alns is None:
        L = MM.lib()
        wb = L.gbx_mm_paf_workspace_bytes(n, reg_cap)
        work = torch.empty(max(wb, 1), dtype=torch.uint8, device=d)
        N.check(L.gbx_mm_paf_device(n, g, ro, n_regs, reg_cap, qn, qo, so, rep, len(tnames), tn, to_, tso, out.data_ptr(), text_cap, lo.data_ptr(),
                                    nt.data_ptr(), work.data_ptr(), wb, s))
    else:
        L = MA.lib()
        wb = L.gbx_mm_paf_cigar_workspace_bytes(n, reg_cap)
        work = torch.empty(max(wb, 1), dtype=torch.uint8, device=d)
        ta, tc = t(alns, MA.ALN_DTYPE, reg_cap), t(cigar, np.uint32)
        N.check(L.gbx_mm_paf_cigar_device(n, g, ro, n_regs, reg_cap, ta.data_ptr(), tc.data_ptr(), len(cigar), qn, qo, so, rep, len(tnames), tn, to_, tso,
                                          out.data_ptr(), text_cap, lo.data_ptr(), nt.data_ptr(), work.data_ptr(), wb, s))
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    return dict(text=o[:text_cap].tobytes(), n_text=int(nt.item()), line_off=lo.cpu().numpy(), intact=bool((o[text_cap:] == 0x5a).all()))
