"""Sequential restatement of minimap2's seeding stage: the minimizer sketch (mm_sketch), the minimizer index
(mm_idx_*) and seed collection with the occurrence filter (collect_matches + collect_seed_hits).  Plain Python integers, one
base at a time; this file pins the device code (minimap2's source is not part of the reference tree)."""
import numpy as np

M64 = (1 << 64) - 1
INT32_MAX = 0x7fffffff
SEED_TANDEM = 1 << 42


def code(ch):
    """A/C/G/T -> 0..3 in either case; anything else 4 (ambiguous).  ch: a byte value."""
    return {65: 0, 97: 0, 67: 1, 99: 1, 71: 2, 103: 2, 84: 3, 116: 3}.get(ch, 4)


def hash64(key, mask):
    """minimap2's invertible integer mix, all of it masked to 2k bits."""
    key = (~key + (key << 21)) & mask
    key = key ^ key >> 24
    key = ((key + (key << 3)) + (key << 8)) & mask
    key = key ^ key >> 14
    key = ((key + (key << 2)) + (key << 4)) & mask
    key = key ^ key >> 28
    key = (key + (key << 31)) & mask
    return key


def sketch(seq, w, k, rid=0, is_hpc=False, stats=None):
    """-> [(x, y)] in the order the sequential machine pushes them.  seq: bytes.  stats: a dict that receives `symmetric`,
    the number of k-mers skipped because they equal their reverse complement."""
    assert 1 <= w <= 255 and 1 <= k <= 28
    if isinstance(seq, str):
        seq = seq.encode()
    n = len(seq)
    mask, shift1 = (1 << 2 * k) - 1, 2 * (k - 1)
    NONE = (M64, M64)
    buf = [NONE] * w
    mn, min_pos, buf_pos, l = NONE, 0, 0, 0
    f = r = 0
    q, span = [], 0                                  # the last k run lengths (HPC) and their sum
    out = []
    n_sym = 0
    i = 0
    while i < n:
        c = code(seq[i])
        info = NONE
        if c < 4:
            if is_hpc:
                run = 1
                while i + run < n and code(seq[i + run]) == c:
                    run += 1
                i += run - 1                         # i: the run's last base
                q.append(run)
                span += run
                if len(q) > k:
                    span -= q.pop(0)
            else:
                span = l + 1 if l + 1 < k else k
            f = (f << 2 | c) & mask
            r = r >> 2 | (3 ^ c) << shift1
            if f == r:                               # symmetric: no slot, no ++l, no buffer write
                n_sym += 1
                i += 1
                continue
            z = 0 if f < r else 1
            l += 1
            if l >= k and span < 256:
                info = (hash64(r if z else f, mask) << 8 | span, rid << 32 | (i & 0xffffffff) << 1 | z)
        else:
            l, q, span = 0, [], 0
        buf[buf_pos] = info
        ring = list(range(buf_pos + 1, w)) + list(range(0, buf_pos))           # ring order, without the slot just written
        if l == w + k - 1 and mn[0] != M64:                                     # (a) the first full window
            out += [buf[j] for j in ring if buf[j][0] == mn[0] and buf[j][1] != mn[1]]
        if info[0] <= mn[0]:                                                    # (b) a new minimum
            if l >= w + k and mn[0] != M64:
                out.append(mn)
            mn, min_pos = info, buf_pos
        elif buf_pos == min_pos:                                                # (c) the minimum leaves the ring
            if l >= w + k - 1 and mn[0] != M64:
                out.append(mn)
            mn = (M64, mn[1])
            for j in ring + [buf_pos]:
                if mn[0] >= buf[j][0]:
                    mn, min_pos = buf[j], j
            if l >= w + k - 1 and mn[0] != M64:
                out += [buf[j] for j in ring + [buf_pos] if buf[j][0] == mn[0] and buf[j][1] != mn[1]]
        buf_pos = buf_pos + 1 if buf_pos + 1 < w else 0
        i += 1
    if mn[0] != M64:
        out.append(mn)
    if stats is not None:
        stats["symmetric"] = n_sym
    return out


def unpack(m):
    """(x, y) -> (hash, span, pos, strand)"""
    return m[0] >> 8, m[0] & 0xff, (m[1] & 0xffffffff) >> 1, m[1] & 1


def mid_occ_of(counts, frac, explicit=0):
    """The occurrence threshold of an index whose keys have these counts.  frac: as float32, as the C struct holds it."""
    if explicit > 0:
        return explicit
    f = float(np.float32(frac))
    if f <= 0.0 or len(counts) == 0:
        return INT32_MAX
    return sorted(counts)[int((1.0 - f) * len(counts)) & 0xffffffff] + 1


class Index:
    """keys ascending; vals[key]: its y values ascending."""

    def __init__(self, seqs, w, k, is_hpc=False, mid_occ=0, mid_occ_frac=2e-4):
        self.w, self.k, self.is_hpc = w, k, is_hpc
        self.vals = {}
        for rid, s in enumerate(seqs):
            if len(s) == 0 or len(s) < k:
                continue
            for x, y in sketch(s, w, k, rid, is_hpc):
                self.vals.setdefault(x >> 8, []).append(y)
        for v in self.vals.values():
            v.sort()
        self.keys = sorted(self.vals)
        self.mid_occ = mid_occ_of([len(self.vals[key]) for key in self.keys], mid_occ_frac, mid_occ)

    def flat(self):
        """(keys uint64, koff int64, vals uint64): the CSR form"""
        koff = np.zeros(len(self.keys) + 1, dtype=np.int64)
        for i, key in enumerate(self.keys):
            koff[i + 1] = koff[i] + len(self.vals[key])
        vals = [y for key in self.keys for y in self.vals[key]]
        return np.array(self.keys, dtype=np.uint64), koff, np.array(vals, dtype=np.uint64)


def seed(idx, read, max_gap=5000, bw=500):
    """One query read -> dict(mini, ax, ay, rep_len, hdr) with hdr = (avg_qspan float32, max_dist_x, max_dist_y, bw, n_segs).
    Anchors ascending by (x, y): minimap2 sorts by x alone, unstably; the tie is broken by the whole of y."""
    if isinstance(read, str):
        read = read.encode()
    qlen = len(read)
    mv = sketch(read, idx.w, idx.k, 0, idx.is_hpc)
    a = []
    rep_st = rep_en = rep_len = 0
    for i, (x, y) in enumerate(mv):
        q_pos, q_span = y & 0xffffffff, x & 0xff
        vals = idx.vals.get(x >> 8, [])
        if len(vals) >= idx.mid_occ:
            en = (q_pos >> 1) + 1
            st = en - q_span
            if st > rep_en:
                rep_len += rep_en - rep_st
                rep_st, rep_en = st, en
            else:
                rep_en = en
            continue
        tandem = (i > 0 and mv[i - 1][0] >> 8 == x >> 8) or (i + 1 < len(mv) and mv[i + 1][0] >> 8 == x >> 8)
        for r in vals:
            rpos = (r & 0xffffffff) >> 1
            if (r & 1) == (q_pos & 1):
                ax = (r & 0xffffffff00000000) | rpos
                ay = q_span << 32 | q_pos >> 1
            else:
                ax = 1 << 63 | (r & 0xffffffff00000000) | rpos
                ay = q_span << 32 | (qlen - ((q_pos >> 1) + 1 - q_span) - 1)
            if tandem:
                ay |= SEED_TANDEM
            a.append((ax, ay))
    rep_len += rep_en - rep_st
    a.sort()
    n = len(a)
    avg = np.float32(0) if n == 0 else np.float32(sum(y >> 32 & 0xff for _, y in a)) / np.float32(n)
    return dict(mini=mv, ax=[x for x, _ in a], ay=[y for _, y in a], rep_len=rep_len,
                hdr=(np.float32(avg), max_gap, max_gap, bw, 1))


def seed_batch(idx, reads, max_gap=5000, bw=500):
    """-> the flat arrays a device call leaves: off, ax, ay, hdr (CHAIN_CALL_DTYPE fields), rep_len, n_mini, mini_off, mini_x, mini_y"""
    rs = [seed(idx, r, max_gap, bw) for r in reads]
    off = np.zeros(len(reads) + 1, dtype=np.int64)
    moff = np.zeros(len(reads) + 1, dtype=np.int64)
    for i, r in enumerate(rs):
        off[i + 1] = off[i] + len(r["ax"])
        moff[i + 1] = moff[i] + len(r["mini"])
    hdr = np.zeros(len(reads), dtype=np.dtype([("avg_qspan", "<f4"), ("max_dist_x", "<i4"), ("max_dist_y", "<i4"), ("bw", "<i4"), ("n_segs", "<i4")]))
    for i, r in enumerate(rs):
        hdr[i] = r["hdr"]
    u = lambda seqs: np.array([v for s in seqs for v in s], dtype=np.uint64)
    return dict(off=off, ax=u(r["ax"] for r in rs), ay=u(r["ay"] for r in rs), hdr=hdr,
                rep_len=np.array([r["rep_len"] for r in rs], dtype=np.int32), n_mini=np.diff(moff).astype(np.int32), mini_off=moff,
                mini_x=u([m[0] for m in r["mini"]] for r in rs), mini_y=u([m[1] for m in r["mini"]] for r in rs))
