"""Inputs of the seed-chaining tests: hand-built hits for every rule of the specification, and a generator of
synthetic reads whose hits need no index (collinear runs on both strands, repeats, noise, bad hits).  A job is a dict of the
arrays the entries take (mem_chain_ref.from_seeds) plus L, contig_off and the parameters that differ from the defaults.
"""
import json
import os

import numpy as np

import mem_chain_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mem_chain_example.json")


def example():
    with open(GOLDEN) as f:
        return json.load(f)


def job(reads, L=1000, contig_off=None, lq=100, **params):
    j = R.from_seeds(reads, lq)
    j.update(L=L, contig_off=np.array(contig_off if contig_off is not None else [0, L], dtype=np.int64), params=params)
    return j


def hand_built():
    """name -> job.  Every read is one rule's edge; the comments give what must happen."""
    ex = [tuple(s) for s in example()["seeds"]]
    J = {}
    J["example"] = job([ex])
    J["example_min_seed_len_10"] = job([ex], min_seed_len=10)
    J["chaining"] = job([
        [(0, 30, 990)],                                              # crosses L: skipped
        [(0, 30, 970), (10, 30, 1000)],                              # ends at L; starts at L (reverse strand): two chains
        [(0, 20, 980), (20, 20, 1000)],                              # a reverse-strand seed next to a forward chain: new chain
        [(0, 20, 500), (30, 20, 530), (60, 20, 520)],                # y < 0: new chain
        [(0, 20, 500), (30, 20, 630)],                               # y - x = w: appended
        [(0, 20, 500), (30, 20, 631)],                               # y - x = w + 1: new chain
        [(10, 30, 500), (50, 30, 540), (10, 10, 500), (70, 10, 560), (71, 10, 561)],   # contained at both edges, then one past
        [(0, 20, 500), (30, 20, -1), (30, 20, 530)],            # a -1 hit between two seeds of one chain
        [],                                                          # no SMEMs
        [(0, 30, 990), (5, 20, -1), (40, 30, 985)],                  # every hit skipped
        [(0, 20, 1999 - 19), (0, 20, 1981)],                         # the last bases of the text; one past them
    ])
    J["x_minus_y"] = job([[(0, 20, 500), (150, 20, 550)], [(0, 20, 500), (150, 20, 549)]], lq=300)      # x - y = w, w + 1
    J["tie"] = job([[(0, 20, 300), (50, 20, 300), (60, 20, 310)],    # two chains of pos 300: the later one is `lower`
                    [(0, 20, 300), (50, 20, 300), (75, 20, 300), (80, 20, 305)]], w=10)
    J["contigs"] = job([
        [(0, 30, 290)],                                              # crosses the boundary at 300: skipped
        [(0, 30, 270), (40, 30, 300)],                               # contig 0, then contig 1 next to it: two chains
        [(0, 30, 1340)],                                             # reverse strand, [630, 660) forward: crosses 650
        [(0, 30, 1350), (40, 30, 1390)],                             # reverse strand, contig 1
        [(0, 30, 620), (35, 30, 655)],                               # collinear across the boundary at 650: two chains
    ], contig_off=[0, 300, 650, 1000])
    J["max_chain_gap"] = job([
        [(0, 20, 500), (69, 20, 569)], [(0, 20, 500), (70, 20, 570)],            # query side: gap 49 / 50
        [(0, 20, 500), (30, 20, 569)], [(0, 20, 500), (30, 20, 570)],            # reference side: gap 49 / 50
    ], max_chain_gap=50)
    flt = [
        [(0, 20, 500), (30, 30, 2000), (70, 25, 3000)],              # weights 20, 30, 25
        [(0, 30, 5000), (10, 30, 2000), (20, 30, 3000), (70, 30, 1000), (25, 30, 8000 + 10000)],      # equal weights
        [(0, 100, 5000), (10, 30, 2000), (50, 28, 3000)],            # B stopped and rescued through A.first, C stopped and gone
        [(0, 100, 5000), (10, 30, 2000), (50, 28, 3000), (120, 60, 7000), (125, 30, 12000), (130, 20, 900)],
    ]
    J["filter"] = job(flt, L=10000, lq=200)
    J["filter_min_weight"] = job(flt, L=10000, lq=200, min_chain_weight=25)
    ext = [ex + [(40, 24, 400)], ex, [(0, 30, 100), (5, 30, 300), (10, 30, 500), (15, 30, 700), (20, 30, 900), (60, 35, 1200)]]
    J["max_chain_extend_1"] = job(ext, max_chain_extend=1)
    J["max_chain_extend_2"] = job(ext, max_chain_extend=2)
    J["mask_level"] = job([
        [(0, 30, 200), (21, 40, 600)],                               # overlap 9 of min_l 30: 9 >= 30 * 0.3f is false in fp32
        [(0, 30, 200), (20, 40, 600)],                               # overlap 10
        [(0, 40, 200), (37, 10, 600)],                               # overlap 3 of min_l 10: 3 >= 10 * 0.3f is false in fp32
        [(0, 40, 200), (36, 10, 600)],
    ], mask_level=0.3)
    win = [
        [(0, 100, 500)],                                             # qbeg = 0 and qbeg + len = lq: gap() of a negative numerator
        [(50, 20, 10)],                                              # clamped at 0
        [(0, 20, 1975)],                                             # clamped at 2 L
        [(0, 20, 950)],                                              # forward, cut at L
        [(60, 20, 1010)],                                            # reverse, cut at L
        [(10, 20, 400), (50, 25, 441), (80, 20, 470)],
    ]
    J["window"] = job(win)
    J["window_scoring"] = job(win, a=2, o_del=4, e_del=2, o_ins=8, e_ins=3, w=30)
    J["window_contig"] = job([[(40, 20, 410)], [(40, 20, 1560)], [(0, 20, 400)], [(80, 20, 430)]], contig_off=[0, 400, 450, 1000])
    return J


def synthetic(n_reads, seed, L=20000, contig_off=None, lq=151, many=()):
    """Reads whose SMEMs and hits are made up: per read a few loci (either strand), each a collinear run of seeds with a
    little diagonal jitter; SMEMs shared by loci get one hit each (several hits per SMEM), some SMEMs hit random places, some
    hits are -1, some SMEMs carry s above max_occ.  Reads in `many` get hundreds of scattered single-hit SMEMs (more than
    64 chains).  SMEMs come sorted by (m, -n) as the SMEM search delivers them."""
    rng = np.random.default_rng(seed)
    co = np.array(contig_off if contig_off is not None else [0, L], dtype=np.int64)
    m, n, s, pos, smem_off, pos_off = [], [], [], [], [0], [0]
    for r in range(n_reads):
        sm = {}
        if r in many:
            for _ in range(int(rng.integers(200, 400))):
                q = int(rng.integers(0, lq - 19))
                ln = int(rng.integers(19, min(40, lq - q) + 1))
                sm.setdefault((q, ln), []).append(int(rng.integers(0, 2 * L - ln)))
        elif r % 17 != 3:
            for _ in range(int(rng.integers(1, 5))):
                base = int(rng.integers(0, 2 * L - lq))
                q = int(rng.integers(0, 30))
                while q < lq - 19:
                    ln = int(rng.integers(19, min(60, lq - q) + 1))
                    if rng.random() < 0.8:
                        sm.setdefault((q, ln), []).append(base + q + int(rng.integers(-3, 4)) * int(rng.random() < 0.3))
                    q += int(rng.integers(5, 50))
            for _ in range(int(rng.integers(0, 4))):
                q = int(rng.integers(0, lq - 19))
                ln = int(rng.integers(19, min(40, lq - q) + 1))
                sm.setdefault((q, ln), []).extend(int(x) for x in rng.integers(-1, 2 * L - ln, int(rng.integers(1, 12))))
        for (q, ln) in sorted(sm, key=lambda k: (k[0], -(k[0] + k[1]))):
            hits = sm[(q, ln)]
            m.append(q)
            n.append(q + ln - 1)
            s.append(len(hits) if rng.random() < 0.9 else 501 + len(hits))
            pos.extend(max(-1, h) for h in hits)
            pos_off.append(len(pos))
        smem_off.append(len(m))
    j = dict(m=np.array(m, dtype=np.int64), n=np.array(n, dtype=np.int64), s=np.array(s, dtype=np.int64),
             smem_off=np.array(smem_off, dtype=np.int64), pos=np.array(pos, dtype=np.int64), pos_off=np.array(pos_off, dtype=np.int64),
             read_off=np.arange(n_reads, dtype=np.int64) * lq, read_len=np.full(n_reads, lq, dtype=np.int32), L=L, contig_off=co,
             params={})
    return j


def reference(j, lookup="bisect", **override):
    P = R.params(**dict(j["params"], **override))
    return R.chain_all(j["m"], j["n"], j["s"], j["smem_off"], j["pos"], j["pos_off"], j["read_off"], j["read_len"], j["L"],
                       j["contig_off"], P, lookup)


def same(got, want):
    """Bit-exact on chains, chain_off, seeds and l_rep; names the first difference."""
    for k in ("chain_off", "l_rep", "chains", "seeds"):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, "%s: %s against %s" % (k, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bad = int(np.nonzero(g != w)[0][0])
            raise AssertionError("%s differs at %d: got %s want %s" % (k, bad, g[bad], w[bad]))
