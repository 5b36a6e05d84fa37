"""CPU restatement of the whole-seed extension (TEST INFRASTRUCTURE): bwa's mem_chain2aln extension logic written out with
numpy over a whole batch, once per side and band try.  Each ksw step is a batched call of a pair extender - by default the
oracle (oracle_py.bsw_oracle, scalarBandedSWA) - on the seeds that side and try extends, with band w << i and the side's end
bonus.  The semantics are those of include/gbx.h (bsw: seeds).

`ksw(params, BswBatch) -> int32[m, 6]` may be replaced (scripts/time_bsw_seeds.py runs the same composition on the GPU's
pair entry); `stats` collects per side and try the pairs extended and their nominal cells (sum of qlen * tlen)."""
import ctypes as C

import numpy as np

from genomicsbench_amd.bsw import BswBatch
from oracle import oracle_py as O

SCORE, TLE, GTLE, QLE, GSCORE, MAX_OFF = range(6)


def oracle_ksw(nthreads=4):
    return lambda params, b: O.bsw_oracle(params, b, nthreads)


def _pair_params(p, w, end_bonus):
    q = type(p.bsw)()
    C.memmove(C.byref(q), C.byref(p.bsw), C.sizeof(q))
    q.w, q.end_bonus = w, end_bonus
    return q


def _side(p, ref, qer, idr, idq, tlen, qlen, h0, active, score, pen, ksw, stats, name):
    """The band-retry loop of one side over the seeds in `active`; `score` (the running score) is updated in place.
    Returns the last try's results (int32[n, 6], rows of inactive seeds undefined) and each seed's last band."""
    n = len(score)
    res = np.zeros((n, 6), dtype=np.int32)
    aw = np.full(n, p.bsw.w, dtype=np.int32)
    todo = np.nonzero(active)[0]
    for i in range(p.max_band_try):
        if todo.size == 0:
            break
        w = p.bsw.w << i
        b = BswBatch(ref, qer, idr[todo], idq[todo], tlen[todo], qlen[todo], h0[todo])
        r = ksw(_pair_params(p, w, pen), b)
        if stats is not None:
            stats.setdefault(name, []).append(dict(pairs=int(todo.size), cells=b.nominal_cells))
        prev = score[todo].copy()
        score[todo] = r[:, SCORE]
        res[todo] = r
        aw[todo] = w
        again = (r[:, SCORE] != prev) & (r[:, MAX_OFF] >= (w >> 1) + (w >> 2))
        todo = todo[again]
    return res, aw


def extend_seeds_ref(p, batch, ksw=None, stats=None):
    """-> int32[n, 8] in the order of bsw_seeds.SEED_RESULT_FIELDS."""
    ksw = ksw or oracle_ksw()
    s = batch.seeds
    n = batch.n
    a = int(p.bsw.mat[0])
    qoff, roff = s["qoff"].astype(np.int64), s["roff"].astype(np.int64)
    lq, rlen, qbeg, rbeg, ln = (s[f].astype(np.int64) for f in ("lq", "rlen", "qbeg", "rbeg", "len"))
    q0, r0 = qbeg + ln, rbeg + ln
    i32 = lambda x: np.ascontiguousarray(x, dtype=np.int32)
    out = np.zeros((n, 8), dtype=np.int32)
    score = np.full(n, -1, dtype=np.int64)
    # left: the reversed prefixes, i.e. slices of the reversed arenas
    rref, rqer = batch.ref[::-1].copy(), batch.qer[::-1].copy()
    left = qbeg > 0
    res, aw0 = _side(p, rref, rqer, batch.ref.size - roff - rbeg, batch.qer.size - qoff - qbeg, i32(rbeg), i32(qbeg),
                     i32(ln * a), left, score, p.pen_clip5, ksw, stats, "left")
    g, sc = res[:, GSCORE].astype(np.int64), res[:, SCORE].astype(np.int64)
    local = (g <= 0) | (g <= sc - p.pen_clip5)
    qb = np.where(left, np.where(local, qbeg - res[:, QLE], 0), 0)
    rb = np.where(left, np.where(local, rbeg - res[:, TLE], rbeg - res[:, GTLE]), rbeg)
    truesc = np.where(left, np.where(local, sc, g), ln * a)
    score = np.where(left, score, ln * a)
    sc0 = score.copy()
    # right: forward suffixes, h0 = the left score
    right = q0 != lq
    res, aw1 = _side(p, batch.ref, batch.qer, roff + r0, qoff + q0, i32(rlen - r0), i32(lq - q0), i32(sc0), right, score,
                     p.pen_clip3, ksw, stats, "right")
    g, sc = res[:, GSCORE].astype(np.int64), res[:, SCORE].astype(np.int64)
    local = (g <= 0) | (g <= sc - p.pen_clip3)
    qe = np.where(right, np.where(local, q0 + res[:, QLE], lq), lq)
    re = np.where(right, np.where(local, r0 + res[:, TLE], r0 + res[:, GTLE]), r0)
    truesc = truesc + np.where(right, np.where(local, sc, g) - sc0, 0)
    for k, v in enumerate((score, truesc, qb, qe, rb, re, np.maximum(aw0, aw1), sc0)):
        out[:, k] = v
    return out
