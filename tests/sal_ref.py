"""Restatement of the suffix-array lookup (include/gbx.h, gbx_fmi_sal_*) over the host tables, in numpy: which rows of an SMEM
are its hits (bwa-mem's mem_chain sampling) and the LF walk from a row to a sampled row or the sentinel row."""
import numpy as np


def hit_rows(k, s, max_occ):
    """rows k + i step, i = 0, 1, ... while i step < s and i < max_occ (max_occ <= 0: every row) of every SMEM -> (rows, off)."""
    k = np.asarray(k, dtype=np.int64)
    s = np.asarray(s, dtype=np.int64)
    if max_occ > 0:
        cnt = np.minimum(s, max_occ)
        step = np.where(s > max_occ, s // max_occ, 1)
    else:
        cnt, step = s, np.ones_like(s)
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    i = np.arange(off[-1], dtype=np.int64) - np.repeat(off[:-1], cnt)
    return np.repeat(k, cnt) + i * np.repeat(step, cnt), off


def sa_walk(index, samples, rows, return_steps=False):
    """SA[r] of every row: while r is not sampled (and not the sentinel row), r <- count[b] + occ_b(r), t += 1."""
    idx = index.host()
    smp = samples.values()
    cx = samples.sa_compx
    mask = (1 << cx) - 1
    cnt = np.asarray(idx.count, dtype=np.int64)
    cpc = idx.cp_occ["cp_count"].astype(np.int64)
    oh = idx.cp_occ["one_hot_bwt_str"].astype(np.uint64)
    r = np.asarray(rows, dtype=np.int64).copy()
    t = np.zeros(len(r), dtype=np.int64)
    out = np.full(len(r), -1, dtype=np.int64)
    act = np.arange(len(r))
    while len(act):
        rr = r[act]
        samp = (rr & mask) == 0
        sent = rr == idx.sentinel_index
        done = samp | sent
        out[act[samp]] = smp[rr[samp] >> cx] + t[act[samp]]
        ds = sent & ~samp
        out[act[ds]] = t[act[ds]]
        act, rr = act[~done], rr[~done]
        if not len(act):
            break
        q, y = rr >> 6, (rr & 63).astype(np.uint64)
        w = oh[q]                                                       # (m, 4)
        bits = (w >> (np.uint64(63) - y)[:, None]) & np.uint64(1)
        assert np.all(bits.sum(1) == 1), "a row other than the sentinel's must have exactly one BWT symbol"
        b = np.argmax(bits, axis=1)
        ww = w[np.arange(len(b)), b]
        m = np.where(y > 0, ~np.uint64(0) << (np.uint64(64) - np.maximum(y, np.uint64(1))), np.uint64(0))
        occ = cpc[q, b] + np.bitwise_count(ww & m).astype(np.int64)
        r[act] = cnt[b] + occ
        t[act] += 1
    return (out, t) if return_steps else out


def smem_positions(index, samples, k, s, max_occ):
    """(pos, pos_off) as gbx_fmi_sal_* return them."""
    rows, off = hit_rows(k, s, max_occ)
    return sa_walk(index, samples, rows), off
