"""Plain Python / numpy restatement of Flye's minimizer index as the reference kmer-cnt builds it with use_minimizers = 1
(R/benchmarks/kmer-cnt: kmer.h:206-262 yieldMinimizers, vertex_index.cpp:389-497 buildIndexMinimizers and 173-212
filterFrequentKmers, sequence_container.cpp globalPosition).  The oracle of the kmer index tests: the deque is restated
literally, with none of the product's reasoning about it (csrc/kmer_index_rules.h)."""
from collections import deque

import numpy as np

MASK64 = (1 << 64) - 1


def splitmix64(x):
    """Kmer::hash (kmer.h:91-98)."""
    z = (x + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def read_kmers(codes, k):
    """-> (canonical codes, reversed flags) of positions 0 .. len - k - 1 (IterKmers stops before the last window); a base
    byte counts with its low two bits; reversed only if revcomp < forward (standardForm)."""
    c = [int(v) & 3 for v in codes]
    n = len(c) - k
    canon, rev = [], []
    if n <= 0:
        return canon, rev
    mask = (1 << (2 * k)) - 1
    f = r = 0
    for i, b in enumerate(c[:n + k - 1]):
        f = ((f << 2) | b) & mask
        r = (r >> 2) | ((3 - b) << (2 * (k - 1)))
        if i >= k - 1:
            canon.append(min(f, r))
            rev.append(r < f)
    return canon, rev


def minimizers_deque(hashes, w):
    """yieldMinimizers over the hashes of a read's positions -> the chosen positions."""
    n = len(hashes)
    if w == 1:
        return list(range(n))
    out = []
    q = deque()                                            # (position, hash)
    for p in range(n):
        h = hashes[p]
        while q and q[-1][1] > h:
            q.pop()
        q.append((p, h))
        if q[0][0] <= p - w:
            while q[0][0] <= p - w:
                q.popleft()
            while len(q) >= 2 and q[0][1] == q[1][1]:
                q.popleft()
        if not out or out[-1] != q[0][0]:
            out.append(q[0][0])
    return out


def read_minimizers(codes, k, w):
    """-> (positions, reversed flags, canonical codes) of one read's minimizers."""
    canon, rev = read_kmers(codes, k)
    pos = minimizers_deque([splitmix64(c) for c in canon], w)
    return pos, [rev[p] for p in pos], [canon[p] for p in pos]


def minimizers_ref(reads, k, w):
    """reads: a KmerReadSet -> (mini_off int64[n_reads + 1], mini_pos int32[], mini_rev uint8[])."""
    off, pos, rev = [0], [], []
    for o, n in zip(reads.read_off.tolist(), reads.read_len.tolist()):
        p, r, _ = read_minimizers(reads.enc[o:o + n], k, w)
        pos.extend(p)
        rev.extend(r)
        off.append(len(pos))
    return np.array(off, dtype=np.int64), np.array(pos, dtype=np.int32), np.array(rev, dtype=np.uint8)


def filter_scalar(total, unique, rate):
    """filterFrequentKmers: (mean as float32, repetitive frequency).  fp32 throughout, the product truncated (the float is
    assigned to a size_t member)."""
    mean = np.float32(total) / np.float32(unique + 1)
    return mean, int(np.float32(rate) * mean)


def index_ref(reads, k, w, rate):
    """-> (stats dict, kmer uint64[], off int64[], pos uint64[]) as gbx_kmer_index_host returns them."""
    table = {}                                             # canonical code -> global positions
    g = 0
    for o, n in zip(reads.read_off.tolist(), reads.read_len.tolist()):
        p, r, c = read_minimizers(reads.enc[o:o + n], k, w)
        for pi, ri, ci in zip(p, r, c):
            table.setdefault(ci, []).append(g + n + (n - pi - k) if ri else g + pi)
        g += 2 * n
    total = sum(len(v) for v in table.values())
    mean, rf = filter_scalar(total, len(table), rate)
    kept = sorted(c for c, v in table.items() if not len(v) > rf)
    kmer = np.array(kept, dtype=np.uint64)
    off = np.zeros(len(kept) + 1, dtype=np.int64)
    pos = []
    for j, c in enumerate(kept):
        pos.extend(sorted(table[c]))
        off[j + 1] = len(pos)
    st = dict(n_chosen=total, n_distinct=len(table), repetitive_frequency=rf, n_repetitive_kmers=len(table) - len(kept),
              n_repetitive_entries=total - len(pos), n_selected=len(kept), n_entries=len(pos), total_len=g // 2,
              mean_frequency=mean)
    return st, kmer, off, np.array(pos, dtype=np.uint64)


def debug_lines(st):
    """The reference's seven --debug lines of buildIndexMinimizers for the stats of an index; floats as its ostream prints
    them (%g of a float)."""
    f32 = np.float32
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = f32(st["n_repetitive_entries"]) / f32(st["n_chosen"])
        mean2 = f32(st["n_entries"]) / f32(st["n_selected"])
        rate = f32(st["total_len"]) / f32(st["n_entries"])
    return ["Mean k-mer frequency: %g" % f32(st["mean_frequency"]),
            "Repetitive k-mer frequency: %d" % st["repetitive_frequency"],
            "Filtered %d repetitive k-mers (%g)" % (st["n_repetitive_entries"], ratio),
            "Selected k-mers: %d" % st["n_selected"],
            "K-mer index size: %d" % st["n_entries"],
            "Mean k-mer frequency: %g" % mean2,
            "Minimizer rate: %g" % rate]
