"""The calls of the kmer index tests, by the edge each one is named for (tests/test_kmer_index_cpu.py holds them against the
host build of the rules header, tests/test_kmer_index_gpu.py against the device).  The tiling constants are restated here;
the CPU test holds them against csrc/kmer_index_rules.h.  A case whose name claims an event at a position is built by search
with the instrumented deque below, so the claim is true of the reference's own walk."""
from collections import deque, namedtuple

import numpy as np

from genomicsbench_amd.kmer import KmerReadSet
import kmer_index_ref as R

KI_LANE, KI_WAVE, KI_TILE, KI_MAX_WINDOW, KI_MAX_K = 8, 512, 2048, 64, 31

Case = namedtuple("Case", "name reads k w rate")
BIG_RATE = 1048576.0            # nothing is repetitive


def rand_read(rng, n):
    return rng.integers(0, 4, n).astype(np.uint8)


def revcomp(a):
    return (3 - np.asarray(a, dtype=np.uint8))[::-1].copy()


def hashes(codes, k):
    return [R.splitmix64(c) for c in R.read_kmers(codes, k)[0]]


def deque_events(h, w):
    """The reference's deque over hashes h (w >= 2), instrumented -> dict of position lists: 'front' the minimizers, 'expiry'
    the steps at which the front expired, 'tie_expiry' those of them whose arriving hash equals the expired front's."""
    ev = dict(front=[], expiry=[], tie_expiry=[])
    q = deque()
    for p, x in enumerate(h):
        while q and q[-1][1] > x:
            q.pop()
        q.append((p, x))
        if q[0][0] <= p - w:
            ev["expiry"].append(p)
            if q[0][1] == x:
                ev["tie_expiry"].append(p)
            while q[0][0] <= p - w:
                q.popleft()
            while len(q) >= 2 and q[0][1] == q[1][1]:
                q.popleft()
        if not ev["front"] or ev["front"][-1] != q[0][0]:
            ev["front"].append(q[0][0])
    return ev


def resets(h, w):
    """positions whose hash is strictly below the w - 1 hashes before them"""
    return [s for s in range(len(h)) if all(h[j] > h[s] for j in range(max(0, s - w + 1), s))]


def read_with_event(rng, kind, x, k, w, tail=80):
    """A read in which an event of `kind` ('reset', 'expiry', 'tie_expiry') happens at position / step x: a long random read
    is cut so that one of its events lands there, and the cut read is checked again."""
    for _ in range(200):
        s = rand_read(rng, x + k + tail + 4 * w + 64)
        h = hashes(s, k)
        found = resets(h, w) if kind == "reset" else deque_events(h, w)[kind]
        for e in found:
            if e < x:
                continue
            cut = s[e - x:e - x + x + k + tail]
            hc = hashes(cut, k)
            got = resets(hc, w) if kind == "reset" else deque_events(hc, w)[kind]
            if x in got:
                return cut
    raise AssertionError("no %s at %d found" % (kind, x))


def read_with_run_end(rng, x, k, tail=80):
    """A homopolymer run of 3 k + 40 bases whose last all-A k-mer is at position x, between other bases."""
    run = 3 * k + 40
    start = x + k - run                                 # the run's first base
    pre = rand_read(rng, max(start, 0))
    if pre.size:
        pre[-1] = 1
    post = rand_read(rng, tail)
    post[0] = 2
    return np.concatenate([pre, np.zeros(run if start >= 0 else run + start, dtype=np.uint8), post])


def ties_cases():
    rng = np.random.default_rng(11)
    k, w = 5, 5
    out = [Case("ties-homopolymers", [np.zeros(n + k, dtype=np.uint8) for n in (1, w - 1, w, w + 1, 3 * w + 2, 3 * KI_TILE)], k, w, BIG_RATE)]
    out.append(Case("ties-tandem", [np.tile(rand_read(rng, p), 300 // p + 2) for p in range(1, w + 2)], k, w, BIG_RATE))
    out.append(Case("ties-palindromes", [np.tile(np.array(u, dtype=np.uint8), 60) for u in ([0, 3], [1, 2], [0, 3, 1, 2])], 2, 4, BIG_RATE))
    both = []
    for _ in range(6):
        u = rand_read(rng, 5)
        both.append(np.concatenate([rand_read(rng, 20), u, rand_read(rng, int(rng.integers(0, 3))), revcomp(u), rand_read(rng, 20)]))
    out.append(Case("ties-both-strands-in-a-window", both, 5, 8, BIG_RATE))
    out.append(Case("ties-equal-hash-at-expiry", [read_with_event(rng, "tie_expiry", x, 2, 3, tail=30) for x in (3, 7, 20)], 2, 3, BIG_RATE))
    return out


def tiles_cases():
    rng = np.random.default_rng(12)
    out = []
    k, w = 3, 4                                          # few k-mers: ties, expiries and resets are all frequent
    for name, b in (("lane", KI_LANE), ("wave", KI_WAVE), ("tile", KI_TILE)):
        reads = []
        for x in (b - 2, b - 1, b):                      # the tile's last position b - 1 and both neighbours
            reads += [read_with_event(rng, "reset", x, k, w), read_with_event(rng, "expiry", x, k, w), read_with_run_end(rng, x, k)]
        out.append(Case("tiles-events-at-%s-end" % name, reads, k, w, BIG_RATE))
    through = np.concatenate([rand_read(rng, 1000), np.zeros(2 * KI_TILE + 500, dtype=np.uint8), rand_read(rng, 1000)])
    out.append(Case("tiles-homopolymer-through-three", [through, 3 - through], 7, 6, BIG_RATE))
    k, w = 6, 5
    short = [np.zeros(0, dtype=np.uint8), rand_read(rng, k), rand_read(rng, k + 1)]
    out.append(Case("tiles-no-reads", [], k, w, BIG_RATE))
    for i, s in enumerate(short):
        out.append(Case("tiles-one-read-len-%s" % ("0", "k", "k+1")[i], [s], k, w, BIG_RATE))
    for i, s in enumerate(short):
        body = rand_read(rng, 70)
        out.append(Case("tiles-two-reads-short-first-%d" % i, [s, body], k, w, BIG_RATE))
        out.append(Case("tiles-two-reads-short-last-%d" % i, [body, s], k, w, BIG_RATE))
    many = [rand_read(rng, int(n)) for n in rng.integers(20, 60, 1025)]
    for i, r0 in enumerate((0, 1, 2)):                   # first, last and in runs
        many[i] = short[r0]
        many[-1 - i] = short[r0]
    for j in range(500, 512):
        many[j] = short[j % 3]
    out.append(Case("tiles-1025-reads-short-ones-first-last-runs", many, k, w, BIG_RATE))
    return out


def parameter_cases():
    rng = np.random.default_rng(13)
    reads = [rand_read(rng, 300), np.tile(rand_read(rng, 3), 60), rand_read(rng, 150)]
    junk = [r | (rng.integers(0, 64, r.size).astype(np.uint8) << 2) for r in reads]
    out = []
    for k in (1, 2, 16, 17, KI_MAX_K):
        for w in (1, 2, 5, 16, KI_MAX_WINDOW):
            out.append(Case("parameters-k%d-w%d%s" % (k, w, "-junk" if (k + w) % 2 else ""), junk if (k + w) % 2 else reads, k, w, 2.5))
    return out


def capacities(reads, k, w):
    t = {}
    for r in reads:
        for c in R.read_minimizers(r, k, w)[2]:
            t[c] = t.get(c, 0) + 1
    return t


def index_cases():
    rng = np.random.default_rng(14)
    out = [Case("index-only-reversed", [np.full(40, 3, dtype=np.uint8), np.array([3, 3, 2, 3, 3, 2, 2, 3, 3, 2, 3], dtype=np.uint8)], 3, 2, BIG_RATE)]
    out.append(Case("index-one-kmer-many-reads-both-strands", [np.full(int(n), 3 * (i % 2), dtype=np.uint8) for i, n in enumerate(rng.integers(5, 60, 40))],
                    4, 3, BIG_RATE))
    for seed in range(100):                               # capacities exactly the repetitive frequency and one above it
        srng = np.random.default_rng(100 + seed)
        reads = [rand_read(srng, 120) for _ in range(3)]
        cap = capacities(reads, 3, 1)
        have = set(cap.values())
        c = next((c for c in sorted(have) if c + 1 in have and c >= 3), None)
        if c is None:
            continue
        mean = R.filter_scalar(sum(cap.values()), len(cap), 1.0)[0]
        rate = float(np.float32((c + 0.5) / float(mean)))
        if R.filter_scalar(sum(cap.values()), len(cap), rate)[1] == c:
            out.append(Case("index-capacity-at-and-above-the-repetitive-frequency", reads, 3, 1, rate))
            break
    assert out[-1].name.startswith("index-capacity")
    out.append(Case("index-everything-repetitive", [rand_read(rng, 200), rand_read(rng, 100)], 5, 3, 0.0))
    out.append(Case("index-filtered-mix", [rand_read(rng, 400), np.zeros(90, dtype=np.uint8), rand_read(rng, 300)], 4, 3, 2.0))
    return out


def all_cases():
    return ties_cases() + tiles_cases() + parameter_cases() + index_cases()


def read_set(case, junk_free=False):
    reads = [np.asarray(r, dtype=np.uint8) & (3 if junk_free else 255) for r in case.reads]
    return KmerReadSet.from_codes(reads)
