"""CPU restatement of the pileup contract (include/gbx.h, pileup section), written from the contract and not
from the kernels: medaka's calculate_pileup (R/benchmarks/pileup/medaka_counts.c:298-478) over htslib's pileup entries.
Numpy per read.  Test infrastructure only."""
import numpy as np

M, I, D, N, S, H, P, EQ, X = range(9)
REF_OPS = (M, D, N, EQ, X)
QUERY_OPS = (M, I, S, EQ, X)
# nt16 (+16 reverse) -> index in "acgtACGTdD" (medaka_counts.h: num2countbase)
COUNTBASE = np.array([-1, 4, 5, -1, 6, -1, -1, -1, 7, -1, -1, -1, -1, -1, -1, -1,
                      -1, 0, 1, -1, 2, -1, -1, -1, 3, -1, -1, -1, -1, -1, -1, -1], dtype=np.int64)


def _indel(cig, k):
    """htslib resolve_cigar2: the indel at the last position of op k, from the op after it"""
    if k + 1 >= len(cig):
        return 0
    op, op2, l2 = cig[k][0], cig[k + 1][0], cig[k + 1][1]
    if op2 == D and op != D:
        return -l2
    if op2 == I:
        return l2
    if op2 == P and k + 2 < len(cig):
        l3 = 0
        for op3, ln3 in cig[k + 2:]:
            if op3 == I:
                l3 += ln3
            elif op3 in REF_OPS:
                break
        if l3 > 0:
            return l3
    return 0


def _walk(reads, r):
    """per ref-consuming op of read r: (op, ref start, query start, len, indel of its last position)"""
    pos, cig, codes, qual, rev, dt = reads.read(r)
    out, rp, qp = [], pos, 0
    for k, (op, ln) in enumerate(cig):
        if op in REF_OPS:
            out.append((op, rp, qp, ln, _indel(cig, k)))
            rp += ln
        if op in QUERY_OPS:
            qp += ln
    return out, codes, qual, rev, dt


def layout(reads, start, end, num_dtypes=1):
    """-> (pos_col int64[end - start + 1], stats dict as gbx_pileup_layout_stats)"""
    n = end - start
    depth = np.zeros(n + 1, dtype=np.int64)
    max_ins = np.zeros(n, dtype=np.int64)
    aligned, bad = 0, -1
    for r in range(reads.n_reads):
        ops, _, _, _, dt = _walk(reads, r)
        if not ops:
            continue
        r0, r1 = ops[0][1], ops[-1][1] + ops[-1][3]
        lo, hi = max(r0, start), min(r1, end)
        if lo < hi:
            depth[lo - start] += 1
            depth[hi - start] -= 1
        entry = False
        for op, b, _, ln, ind in ops:
            last = b + ln - 1
            if ln > 0 and ind > 0 and start <= last < end:
                max_ins[last - start] = max(max_ins[last - start], ind)
            ov = max(0, min(b + ln, end) - max(b, start))
            if op in (M, EQ, X):
                aligned += ov
            if op != N and ov > 0:
                entry = True
        if entry and num_dtypes > 1 and not (0 <= dt < num_dtypes) and bad < 0:
            bad = r
    d = np.cumsum(depth)[:n]
    cols = np.where(d > 0, 1 + max_ins, 0)
    pos_col = np.zeros(n + 1, dtype=np.int64)
    pos_col[1:] = np.cumsum(cols)
    st = dict(n_cols=int(pos_col[-1]), n_positions=int((d > 0).sum()), max_ins=int(max_ins[d > 0].max()) if (d > 0).any() else 0,
              max_depth=int(d.max()) if n else 0, aligned_bases=int(aligned), bad_read=bad)
    return pos_col, st


def counts(reads, start, end, pos_col, num_dtypes=1, num_homop=5, p0=None, p1=None):
    """-> (major int32[c], minor int32[c], counts uint32[c, F]) of the columns of positions [p0, p1)"""
    p0 = start if p0 is None else p0
    p1 = end if p1 is None else p1
    F = 10 * num_dtypes * num_homop
    c0, c1 = int(pos_col[p0 - start]), int(pos_col[p1 - start])
    nc = c1 - c0
    ncols = np.diff(pos_col[p0 - start:p1 - start + 1])
    major = np.repeat(np.arange(p0, p1, dtype=np.int32), ncols)
    minor = (np.arange(nc) - np.repeat(pos_col[p0 - start:p1 - start] - c0, ncols)).astype(np.int32)
    flat = []
    for r in range(reads.n_reads):
        ops, codes, qual, rev, dt = _walk(reads, r)
        if num_dtypes == 1:
            dt = 0
        if not (0 <= dt < num_dtypes):
            continue
        for op, b, q, ln, ind in ops:
            lo, hi = max(b, p0), min(b + ln, p1)
            if lo >= hi or op == N:
                continue
            p = np.arange(lo, hi)
            col = pos_col[p - start] - c0
            if op == D:                                    # deletions: stratum 0, d (reverse) or D (forward)
                flat.append(col * F + dt * num_homop * 10 + (8 if rev else 9))
                continue
            qp = q + (p - b)
            cols_j, q_j = [col], [qp]
            if ind > 0 and lo <= b + ln - 1 < hi:          # the op's last position and the insertion after it
                j = np.arange(1, ind + 1)
                cols_j.append(np.full(ind, col[-1]) + j)
                q_j.append(np.full(ind, qp[-1]) + j)
            cc, qq = np.concatenate(cols_j), np.concatenate(q_j)
            ok = qq < codes.size
            cc, qq = cc[ok], qq[ok]
            bi = COUNTBASE[codes[qq].astype(np.int64) + (16 if rev else 0)]
            strat = np.zeros(qq.size, dtype=np.int64) if num_homop == 1 else np.maximum(0, np.minimum(qual[qq].astype(np.int64), num_homop) - 1)
            good = bi >= 0
            flat.append(cc[good] * F + (dt * num_homop + strat[good]) * 10 + bi[good])
    idx = np.concatenate(flat) if flat else np.zeros(0, dtype=np.int64)
    cnt = np.bincount(idx, minlength=nc * F).astype(np.uint32).reshape(nc, F)
    return major, minor, cnt
