"""Seeded cases for the minimizer seeding stage (tests/mm_ref.py is the restatement).  The generators assert their own coverage,
so a case that stops exercising its path fails here and not silently."""
import functools
import random

import numpy as np

import mm_ref as R

CHUNK = 256                                # GBX_MM_SKETCH_CHUNK: the long reads below must cross it many times
SKETCH_PARAMS = [(10, 15, 0), (10, 19, 1), (19, 19, 0), (1, 28, 0), (255, 3, 0), (3, 3, 0), (2, 4, 0)]      # (w, k, hpc)
SEVENTEEN = b"ACTAGAGGACATTCCGG"


def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n)).encode()


def long_read(rng, n):
    """n random bases with N runs and low-complexity stretches at seeded random offsets"""
    s = bytearray(rand_seq(rng, n))
    for _ in range(max(3, n // 1500)):
        o, ln = rng.randrange(n), rng.choice([1, 2, 40, 300])
        s[o:o + ln] = b"N" * len(s[o:o + ln])
    for _ in range(max(3, n // 1500)):
        o, ln = rng.randrange(n), rng.choice([30, 120, 400])
        unit = rand_seq(rng, rng.choice([1, 2, 3, 7]), "acgt")      # lower case: the codes are the same
        s[o:o + ln] = (unit * (ln // len(unit) + 1))[:len(s[o:o + ln])]
    return bytes(s)


@functools.lru_cache(maxsize=None)
def sketch_batch(w, k, hpc):
    """The sequences of one sketch call: every edge length in three alphabets, the hand cases, and two long reads."""
    rng = random.Random(1000 * w + 10 * k + hpc)
    seqs = []
    for n in (0, 1, k - 1, k, w + k - 2, w + k - 1, w + k):
        for alpha in ("ACGT", "AC"):
            seqs.append(rand_seq(rng, n, alpha))
        seqs.append(b"N" + rand_seq(rng, max(n - 2, 0), "ACGTN") + b"N" if n >= 2 else b"N" * n)
    run = w + k + 5
    seqs.append(b"N" * run + rand_seq(rng, 3 * (w + k)) + b"N" * run + rand_seq(rng, 2 * (w + k), "ACGTN") + b"N" * run)
    seqs.append(SEVENTEEN)
    seqs.append(b"ACGGGGTTTACCCCCCAGTNACGTTTGCAAAAC")
    seqs.append(rand_seq(rng, 60) + b"A" * 300 + rand_seq(rng, 60))          # under HPC: a span of 256 or more
    seqs.append(rand_seq(rng, 200, "AT"))
    seqs.append(b"AT" * 40)                                                  # k = 4: every k-mer is its own reverse complement
    seqs.append(b"ATATATGCGCATTAATCGAT")
    seqs.append(long_read(rng, 5000))
    seqs.append(long_read(rng, 70000))
    assert len(seqs[-2]) > 8 * CHUNK and len(seqs[-1]) > 8 * CHUNK
    return tuple(seqs)


@functools.lru_cache(maxsize=None)
def sketch_expected(w, k, hpc):
    """(mini_x, mini_y, mini_off) of sketch_batch by the restatement, rid = ordinal"""
    xs, ys, off = [], [], [0]
    for rid, s in enumerate(sketch_batch(w, k, hpc)):
        m = R.sketch(s, w, k, rid, bool(hpc))
        xs += [a for a, _ in m]
        ys += [b for _, b in m]
        off.append(len(xs))
    return np.array(xs, dtype=np.uint64), np.array(ys, dtype=np.uint64), np.array(off, dtype=np.int64)


def mutate(rng, s, rate=0.05):
    out = bytearray()
    for c in s:
        u = rng.random()
        if u < rate / 3:
            continue                                         # deletion
        if u < 2 * rate / 3:
            out.append(rng.choice(b"ACGT"))                  # insertion
        out.append(rng.choice(b"ACGT") if 2 * rate / 3 <= u < rate else c)
    return bytes(out)


def revcomp(s):
    return bytes(s[::-1]).translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))


@functools.lru_cache(maxsize=None)
def index_case():
    """Three reference sequences: one below k, one with N runs, one holding a 40-copy tandem repeat."""
    rng = random.Random(4242)
    unit = rand_seq(rng, 37)
    s1 = rand_seq(rng, 9)
    s2 = bytearray(rand_seq(rng, 3000))
    for o, ln in ((0, 3), (700, 60), (1500, 1), (2990, 10)):
        s2[o:o + ln] = b"N" * ln
    s3 = rand_seq(rng, 1500) + unit * 40 + rand_seq(rng, 1500)
    return (s1, bytes(s2), s3)


INDEX_VARIANTS = [dict(mid_occ_frac=2e-4), dict(mid_occ_frac=0.1), dict(mid_occ_frac=0.0), dict(mid_occ=3)]
SEED_PARAMS = dict(k=15, w=10, is_hpc=0, mid_occ=20)


@functools.lru_cache(maxsize=None)
def seed_case():
    """-> (reference sequences, reads, expected dict of the restatement).  The reference: two sequences with a 40-copy repeat of a 37-mer
    and 12 copies of a 7-mer (one minimizer a period: the tandem flag)."""
    rng = random.Random(777)
    unit, unit7 = rand_seq(rng, 37), b"ACGTTCA"
    r0 = rand_seq(rng, 6000) + unit * 40 + rand_seq(rng, 4000) + unit7 * 12 + rand_seq(rng, 3000)
    r1 = rand_seq(rng, 5500)
    refs = (r0, r1)
    t0 = 6000 + 37 * 40 + 4000                               # where the 7-mer repeat starts
    reads = []
    for _ in range(4):
        o, ln = rng.randrange(0, 5000), rng.randrange(400, 1500)
        reads.append(mutate(rng, r0[o:o + ln]))
    for _ in range(3):
        o, ln = rng.randrange(0, 4500), rng.randrange(400, 1000)
        reads.append(mutate(rng, revcomp(r1[o:o + ln])))
    reads.append(r0[5900:6000] + unit * 12 + rand_seq(rng, 50))                  # the repeat: rep_len > 0, skipped minimizers
    seg = r1[1000:1060]
    reads.append(r1[900:1000] + seg + seg + r1[1060:1200])                        # one segment twice: equal x, different y
    reads.append(r0[t0 - 150:t0 + 84 + 150])                                      # across the 7-mer repeat: the tandem flag
    reads.append(rand_seq(rng, 1000))                                             # nothing in common with the reference
    reads.append(b"")
    reads.append(mutate(rng, revcomp(r0[11000:13500])))
    idx = R.Index(refs, SEED_PARAMS["w"], SEED_PARAMS["k"], False, mid_occ=SEED_PARAMS["mid_occ"])
    exp = R.seed_batch(idx, reads)
    ax, ay, off = exp["ax"], exp["ay"], exp["off"]
    per_read = np.diff(off)
    assert (ax >> np.uint64(63)).any(), "no reverse-strand anchor"
    assert any(ax[i] == ax[i + 1] and ay[i] != ay[i + 1] for r in range(len(reads)) for i in range(off[r], off[r + 1] - 1)), "no equal-x tie"
    assert (exp["rep_len"] > 0).any(), "no rep_len"
    assert (ay & np.uint64(R.SEED_TANDEM)).any(), "no tandem flag"
    assert per_read[-3] == 0 and exp["n_mini"][-3] > 0 and per_read[-2] == 0, "the random and the empty read have anchors"
    assert (per_read > 0).sum() >= 10
    return refs, tuple(reads), exp


SORT_TILE = 4096                           # items a block of the radix sort takes (csrc/gbx_internal.h)


@functools.lru_cache(maxsize=None)
def tile_case():
    """-> (reference sequences, reads, expected dict of the restatement) with enough minimizers and anchors for the (u64, u64)
    radix sort to run over several tiles with a ragged last one: index values, keys and anchors each above two tiles."""
    rng = random.Random(9091)
    refs = (rand_seq(rng, 30000), rand_seq(rng, 20000), rand_seq(rng, 7))
    reads = []
    for i in range(24):
        src = refs[i % 2]
        o = rng.randrange(0, len(src) - 4000)
        s = mutate(rng, src[o:o + 4000], 0.01)
        reads.append(revcomp(s) if i % 3 == 0 else s)
    reads.append(b"")
    idx = R.Index(refs, SEED_PARAMS["w"], SEED_PARAMS["k"], False, mid_occ=SEED_PARAMS["mid_occ"])
    exp = R.seed_batch(idx, reads)
    keys, _, vals = idx.flat()
    for n in (len(vals), len(keys), len(exp["ax"])):
        assert n > 2 * SORT_TILE and n % SORT_TILE != 0, n
    assert (exp["ax"] >> np.uint64(63)).any(), "no reverse-strand anchor"
    return refs, tuple(reads), exp
