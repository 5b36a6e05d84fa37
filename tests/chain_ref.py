"""Plain restatement of chain_dp (R/benchmarks/chain/src/host_kernel.cpp:30-94) for one call, that also says which paths of
csrc/chain_kernels.hip the call reaches.  TEST INFRASTRUCTURE ONLY; small inputs, not fast.

chain_dp() returns the reference's five results (score, parent, target, peak, evaluated pairs) and a list of facts in the
kernel's geometry.  The geometry is restated here from the kernel's comments, nothing is imported from it:
  * a call is cut into jobs (chain_jobs below); i is the anchor's index in its job;
  * anchors are computed in blocks of 64, ib = i & ~63; while block ib is computed the anchors >= live0 = ib - R are
    addressed in the LDS ring (R = 512 or 768), older ones in global memory;
  * the look-back j = i-1 .. st is swept in chunks c = 0, 1, ... of 64 lanes, lane l of chunk c is j = i-1-64c-l.
One fact record per (anchor, chunk), see _record().

`mutant` changes one rule of the restatement to a mistake the kernel could make (MUTANTS); the tests use them to show
that a named case would catch that mistake.
"""
import bisect

import numpy as np

MAX_ITER, MAX_SKIP = 5000, 25          # host_kernel.cpp:37-38
RINGS = (512, 768)
M64 = (1 << 64) - 1
MUTANTS = ("no_round",                 # sc -= gap_cost, without (int)(gap_cost * gap_scale + .499)
           "mark_behind_break",        # :89 also for the lanes of the chunk behind the breaking lane
           "improve_behind_break",     # max_f / max_j also from the lanes of the chunk behind the breaking lane
           "nskip_unclamped",          # --n_skip without `if (n_skip > 0)`
           "no_global_hits",           # targets[j] == i is not seen for j < live0 unless the same chunk marked j
           "no_direct_stores",         # targets[parents[j]] = i is lost when parents[j] < live0
           "window_ignores_own_marks",  # chunk 0 sees no targets[j] == i at all
           "clin_fp32",                # dd * .01 * avg_qspan in fp32
           "dq_limit",                 # dq >= max_dist_y / dq >= max_dist_x
           "dr_limit",                 # dr >= max_dist_y
           "bw_limit",                 # dd >= bw
           "max_iter")                 # i - st > max_iter - 1


def _hdr(h):
    h = h.tolist() if hasattr(h, "tolist") else h
    return float(np.float32(h[0])), int(h[1]), int(h[2]), int(h[3]), int(h[4])


def first_pred(x, max_dist_x, max_iter=MAX_ITER):
    """st of every anchor as the reference's running `st` has it (:56-57), 64-bit unsigned arithmetic"""
    xs = [int(v) for v in x]
    add = max_dist_x & M64
    st, out = 0, []
    for i, ri in enumerate(xs):
        while st < i and ri > ((xs[st] + add) & M64):
            st += 1
        if i - st > max_iter:
            st = i - max_iter
        out.append(st)
    return out


def chain_jobs(x, y, hdr, split=True, wide=False):
    """The cut rule of the kernel's header comment -> [(start, n, narrow)] over one call.
    Sorted calls only are cut: per call-relative aligned block of 64 anchors the first i > 0 with st(i) == i starts a job.
    A job is narrow iff its anchors share one upper x word and one segment id (never with `wide`, never for an unsorted call).
    split=False: the call is one job (GBX_CHAIN_NOSPLIT)."""
    xs = [int(v) for v in x]
    ys = [int(v) for v in y]
    n = len(xs)
    is_sorted = all(xs[i - 1] <= xs[i] for i in range(1, n))
    starts = [0]
    if split and is_sorted:
        st = first_pred(xs, _hdr(hdr)[1])
        for b in range(0, n, 64):
            for i in range(max(b, 1), min(b + 64, n)):
                if st[i] == i:
                    starts.append(i)
                    break
    jobs = []
    for k, s in enumerate(starts):
        e = starts[k + 1] if k + 1 < len(starts) else n
        keys = {(xs[i] >> 32, ys[i] >> 48 & 0xff) for i in range(s, e)}
        jobs.append((s, e - s, is_sorted and not wide and len(keys) <= 1))
    return jobs


def _wrap32(v):
    return ((v + (1 << 31)) & 0xffffffff) - (1 << 31)


def _ilog2(v):
    """ilog2_32 (:19-24) elementwise, v > 0 as uint32"""
    r = np.zeros(v.shape, dtype=np.int64)
    v = v.copy()
    for s in (16, 8, 4, 2, 1):
        m = v >= (1 << s)
        r[m] += s
        v[m] >>= s
    return r


def _tier(c, jhi, lo, live0):
    """where the kernel reads chunk c from: lo = its last valid lane's anchor"""
    if c == 0:
        return "window"
    if jhi - 63 >= live0:
        return "ring"
    return "global" if jhi < live0 else ("straddle" if lo < live0 else "ring_tail")


def _record(i, iabs, c, tier, nvalid, st_lane63, live0, nopen=0, shape="quiet", walk_neg=False, nskip_in=0, dec=0, brk=None,
            brk_improver=False, brk_marks=(), marks=(), hits=()):
    """i: index in the job, iabs: in the call (what targets[] holds).  tier: window | ring | straddle | global (ring_tail:
    a last partial chunk that the global loop takes although all its valid lanes are in the ring).  nvalid: lanes with
    j >= st; st_lane63: lane 63 is valid and is st; nopen: lanes that do not `continue`.  shape: quiet | popcount | lead |
    scan over all 64 lanes as the kernel sees them (the lanes behind a break included); walk_neg: n_skip_in + bumps - improvers goes below 0 inside the
    chunk; dec: improvers that found n_skip > 0 and took it down.  brk: breaking lane or None; brk_improver: a lane of
    the chunk behind it has sc > max_f; brk_marks: call-relative parents that lanes of the chunk behind the break would
    mark (the caller tells from the final targets whether that would change them).  marks: (lane, parent in the job,
    'ring' | 'direct') for every targets[parents[j]] = i; hits: (lane, 'same' | 'ring' | 'global') for every bump, by
    where the kernel learns targets[j] == i: this chunk's own marks, else an earlier chunk's through the ring (j >= live0)
    or through global memory."""
    return dict(i=i, iabs=iabs, c=c, tier=tier, nvalid=nvalid, st_lane63=st_lane63, live0=live0, ib=i & ~63, nopen=nopen, shape=shape,
                walk_neg=walk_neg, nskip_in=nskip_in, dec=dec, brk=brk, brk_improver=brk_improver, brk_marks=tuple(brk_marks),
                marks=tuple(marks), hits=tuple(hits))


def chain_dp(x, y, hdr, ring=512, split=True, wide=False, mutant=None, want_facts=True):
    """-> (score, parent, target, peak, pairs, facts, jobs).  facts: list of _record()s, [] without want_facts."""
    assert mutant is None or mutant in MUTANTS
    avg_qspan, max_dist_x, max_dist_y, bw, n_segs = _hdr(hdr)
    xa = np.ascontiguousarray(x, dtype=np.uint64)
    ya = np.ascontiguousarray(y, dtype=np.uint64)
    n = len(xa)
    q = (ya & np.uint64(0xffffffff)).astype(np.uint32).view(np.int32).astype(np.int64)      # (int32_t)a[i].y
    span = (ya >> np.uint64(32) & np.uint64(0xff)).astype(np.int64)
    sid = (ya >> np.uint64(48) & np.uint64(0xff)).astype(np.int64)
    jobs = chain_jobs(xa, ya, hdr, split, wide)
    job_starts = [s for s, _, _ in jobs]
    sts = first_pred(xa, max_dist_x, MAX_ITER - 1 if mutant == "max_iter" else MAX_ITER)
    score = np.zeros(n, dtype=np.int64)
    parent = np.zeros(n, dtype=np.int64)
    target = np.zeros(n, dtype=np.int64)
    peak = np.zeros(n, dtype=np.int64)
    pairs, facts = 0, []
    ge = (lambda a, b: a >= b) if mutant == "dq_limit" else (lambda a, b: a > b)

    for i in range(n):
        st = sts[i]
        js = np.arange(i - 1, st - 1, -1)
        j0 = job_starts[bisect.bisect_right(job_starts, i) - 1]
        irel = i - j0
        live0 = (irel & ~63) - ring
        q_span = int(span[i])
        if len(js):
            # ---- :59-80 for all j at once, the lines in the reference's order
            dr = (xa[i:i + 1] - xa[js]).view(np.int64)
            dq = _wrap32(q[i] - q[js])
            same = sid[js] == sid[i]
            skip = (same & (dr == 0)) | (dq <= 0)
            skip |= (same & ge(dq, max_dist_y)) | ge(dq, max_dist_x)
            dd = _wrap32(np.where(dr > dq, dr - dq, dq - dr))
            skip |= same & ((dd >= bw) if mutant == "bw_limit" else (dd > bw))
            if n_segs > 1:
                skip |= same & ((dr >= max_dist_y) if mutant == "dr_limit" else (dr > max_dist_y))
            min_d = np.where(dq < dr, dq, _wrap32(dr))
            sc = np.where(min_d > q_span, q_span, min_d)
            log_dd = np.where(dd != 0, _ilog2(dd & 0xffffffff), 0)
            if mutant == "clin_fp32":
                c_lin = np.trunc(dd.astype(np.float32) * np.float32(.01) * np.float32(avg_qspan)).astype(np.int64)
            else:
                c_lin = np.trunc(dd.astype(np.float64) * .01 * avg_qspan).astype(np.int64)
            gap = np.where(same, c_lin + (log_dd >> 1), np.where(dr == 0, 0, np.minimum(c_lin, log_dd)))
            sc = sc + (~same & (dr == 0))
            if mutant != "no_round":
                gap = np.trunc(gap.astype(np.float64) * 1.0 + .499).astype(np.int64)
            sc = _wrap32(sc - gap + score[js])
            open_ = np.nonzero(~skip)[0].tolist()             # positions i-1-j of the lanes that do not `continue`
            scl = sc.tolist()
        else:
            open_, scl = [], []

        # ---- :81-89 in order, chunk by chunk
        best, best_j, n_skip, evaluated = q_span, -1, 0, i - st
        nchunks = (len(js) + 63) >> 6
        at = 0
        for c in range(nchunks):
            jhi = i - 1 - 64 * c
            lo = max(st, jhi - 63)
            nvalid = jhi - lo + 1
            tier = _tier(c, jhi - j0, lo - j0, live0)
            st_l63 = nvalid == 64 and lo == st
            end = at
            while end < len(open_) and open_[end] < 64 * (c + 1):
                end += 1
            if end == at:                                     # every lane `continue`s
                if want_facts:
                    facts.append(_record(irel, i, c, tier, nvalid, st_l63, live0, nskip_in=n_skip))
                continue
            nskip_in, walk, walk_min, dec = n_skip, n_skip, n_skip, 0
            improvers, bumps, marks, hits, brk_marks = [], [], [], [], []
            own = set()                                       # anchors this chunk's lanes have marked
            brk, brk_improver, shadow_best = None, False, best
            for pos in open_[at:end]:
                lane, j, s = pos - 64 * c, i - 1 - pos, scl[pos]
                if mutant == "window_ignores_own_marks" and c == 0:
                    hit = False
                elif mutant == "no_global_hits" and j - j0 < live0:
                    hit = j in own
                else:
                    hit = j in own or int(target[j]) == i
                pj = int(parent[j])
                if brk is None:
                    if s > best:
                        best, best_j = s, j
                        if n_skip > 0 or mutant == "nskip_unclamped":
                            n_skip -= 1
                            dec += 1
                        improvers.append(lane)
                        walk -= 1
                    elif hit:
                        bumps.append(lane)
                        hits.append((lane, "same" if j in own else "ring" if j - j0 >= live0 else "global"))
                        walk += 1
                        n_skip += 1
                        if n_skip > MAX_SKIP:
                            brk, evaluated, shadow_best = lane, pos + 1, best
                            if pj >= 0:
                                own.add(pj)                   # the kernel's marks of a chunk do not know about the break
                            walk_min = min(walk_min, walk)
                            continue
                    walk_min = min(walk_min, walk)
                    if pj >= 0:
                        own.add(pj)
                        direct = pj - j0 < live0
                        marks.append((lane, pj - j0, "direct" if direct else "ring"))
                        if not (direct and mutant == "no_direct_stores"):
                            target[pj] = i
                else:
                    # behind the break: the reference has left the loop; what the kernel's lanes see there
                    if s > shadow_best:
                        shadow_best, brk_improver = s, True
                        improvers.append(lane)
                        walk -= 1
                        if mutant == "improve_behind_break":
                            best, best_j = s, j
                    elif hit:
                        bumps.append(lane)
                        walk += 1
                    walk_min = min(walk_min, walk)
                    if pj >= 0:
                        own.add(pj)
                        brk_marks.append(pj)
                        if mutant == "mark_behind_break":
                            target[pj] = i
            at0, at = at, end
            if want_facts:
                shape = ("popcount" if bumps else "quiet") if not improvers else \
                    ("lead" if not bumps or max(improvers) < min(bumps) else "scan")
                facts.append(_record(irel, i, c, tier, nvalid, st_l63, live0, end - at0, shape, walk_min < 0, nskip_in, dec, brk,
                                     brk_improver, brk_marks, marks, hits))
            if brk is not None:
                break
        pairs += evaluated
        score[i], parent[i] = best, best_j                                                   # :91
        peak[i] = peak[best_j] if best_j >= 0 and peak[best_j] > best else best              # :92
    to32 = lambda a: a.astype(np.int32)
    return to32(score), to32(parent), to32(target), to32(peak), pairs, facts, jobs


def chain_calls(off, ax, ay, hdr, **kw):
    """chain_dp over a packed call list -> (score, parent, target, peak, pairs, [facts per call], [jobs per call])"""
    outs, pairs, facts, jobs = [[], [], [], []], 0, [], []
    for c in range(len(off) - 1):
        a, b = int(off[c]), int(off[c + 1])
        r = chain_dp(ax[a:b], ay[a:b], hdr[c], **kw)
        for o, v in zip(outs, r[:4]):
            o.append(v)
        pairs += r[4]
        facts.append(r[5])
        jobs.append(r[6])
    cat = lambda v: np.concatenate(v) if v else np.zeros(0, np.int32)
    return tuple(cat(o) for o in outs) + (pairs, facts, jobs)
