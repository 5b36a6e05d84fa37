"""Named, deterministic chaining calls at the edges of csrc/chain_kernels.hip.  Every case is one call, built by
construction, with a `claim`: a function over the fact list of tests/chain_ref.py that asserts the case reaches the path it
is named for (tests/test_chain_edges_cpu.py runs the claims, tests/test_chain_edges_gpu.py runs the calls on the device).

Building blocks.  Anchors of a call are 3 reference bases apart (DX) unless a case says otherwise.
  filler   query position far above everything else and falling by 5 an anchor: dq <= 0 against every filler before it,
           dq > max_dist against every other anchor: visited (it counts as a pair and takes a lane) and always skipped.
  diag(o)  an anchor on the diagonal x - q = const + o.  Two of them see each other with dd = |o1 - o2| (when dq > 0).
The anchor T under test lies on o = 0; lane numbers below are positions behind T: pos = i - 1 - j, chunk pos // 64."""
import numpy as np

import chain_ref as CR

DX, X0, QN, QF = 3, 1000, 1_000_000, 10_000_000
HDR = (np.float32(15.0), 5000, 5000, 500, 1)
_cache = {}


class Case:
    def __init__(self, name, x, y, hdr, claim, rings=CR.RINGS):
        self.name, self.hdr, self.claim, self.rings = name, hdr, claim, tuple(rings)
        self.x, self.y = np.asarray(x, dtype=np.uint64), np.asarray(y, dtype=np.uint64)

    @property
    def call(self):
        return self.x, self.y, self.hdr

    def ref(self, ring=512, **kw):
        """chain_ref.chain_dp of the call, computed once per setting and shared"""
        key = (self.name, ring, tuple(sorted(kw.items())))
        if key not in _cache:
            _cache[key] = CR.chain_dp(self.x, self.y, self.hdr, ring=ring, **kw)
        return _cache[key]


class Call:
    """anchors in index order"""

    def __init__(self, x0=X0, dx=DX):
        self.x, self.q, self.span, self.seg, self.dx, self.x0 = [], [], [], [], dx, x0
        self.at = x0

    def _put(self, q, span, seg, x=None):
        if x is not None:
            self.at = x
        self.x.append(self.at)
        self.q.append(q)
        self.span.append(span)
        self.seg.append(seg)
        self.at += self.dx
        return len(self.x) - 1

    def filler(self, k=1, x=None):
        for _ in range(k):
            self._put(QF - 5 * len(self.x), 15, 0, x)
            x = None
        return len(self.x) - 1

    def diag(self, o=0, span=15, x=None, q=None):
        xv = self.at if x is None else x
        return self._put(QN + (xv - self.x0) - o if q is None else q, span, 0, x)

    def arrays(self):
        x = np.array(self.x, dtype=np.uint64)
        y = (np.array(self.seg, dtype=np.uint64) << np.uint64(48)) | (np.array(self.span, dtype=np.uint64) << np.uint64(32)) | \
            (np.array(self.q, dtype=np.int64).astype(np.uint64) & np.uint64(0xffffffff))
        return x, y


def recs_of(facts, i):
    return [r for r in facts if r["iabs"] == i]


def one_narrow_job(res, n):
    assert res[6] == [(0, n, True)], res[6]


# ------------------------------------------------------------------------------------------------ length edges
LENGTHS = (1, 63, 64, 65, 511, 512, 513, 575, 576, 577, 640, 641, 767, 768, 769, 831, 832, 833, 896, 897)


def length_case(n):
    """One job of n anchors in which every anchor looks back to anchor 0.  Every 7th anchor lies on one diagonal (a chain
    that breaks 27 members back, in the ring), every 37th on a second one 2000 off (a chain that never breaks: its
    members are bumps down to anchor 0 through every tier, their parents are marked in the ring and, once they have
    left it, by direct stores); the rest are fillers with spans of their own, so that every flushed word is checked."""
    c = Call()
    for k in range(n):
        if k % 7 == 0:
            c.diag(0, 10 + k % 5)
        elif k % 37 == 1:
            c.diag(2000, 9 + k % 7)
        else:
            c.filler()
            c.span[-1] = 1 + k % 200

    def claim(case, ring, res):
        facts = res[5]
        one_narrow_job(res, n)
        assert not any(CR.first_pred(case.x, 5000))          # st == 0 for every anchor
        tiers = {r["tier"] for r in facts}
        assert ("global" in tiers) == (n > ring + 64) and ("straddle" in tiers) == (n > ring + 65), (n, ring, tiers)
        if n > ring + 64 + 38:
            assert any(m[2] == "direct" for r in facts for m in r["marks"])
            assert any(h[1] == "global" for r in facts for h in r["hits"])
        if n >= 7 * 28:
            assert any(r["brk"] is not None and r["tier"] == "ring" for r in facts)
    return Case("len%d" % n, *c.arrays(), HDR, claim)


# ------------------------------------------------------------------------------------------------ look-back edges
def lookback_d(ring):
    return (0, 1, 63, 64, 65, 128, 129, ring - 1, ring, ring + 1, ring + 63, ring + 64, ring + 65)


def lookback_case(d, lane, ring):
    """T at lane `lane` of a block of its job looks back at exactly d anchors.  The farthest of them (st) lies on T's
    diagonal with span 200 and is T's parent; the anchor before it (1 base too far) lies there too with span 250: a
    look-back one lane too long takes it.  Every 61st anchor in between is on a diagonal 300 off with span 3 (a chain
    of bumps that stays below 26), the others are fillers."""
    c = Call()
    ib = 64 * max(-(-(d - lane) // 64), 0)
    if ib + lane < d + 1 or (d == 0 and lane == 63):
        ib += 64
    i = ib + lane
    if d == 0:
        # T looks back at nobody.  At lane 0 that is a cut and T starts a job; at lane 63 the block's cut is taken by
        # its anchor 0, so T is lane 63 of the job that starts there.
        if lane:
            c.filler(ib)
            c.filler(1, x=c.at + 6000)
            c.filler(lane - 2)
        else:
            c.filler(i - 1)
        bait = c.diag(0, 250)
        t = c.diag(0, 15, x=c.at + 6000)
    else:
        c.filler(i - d - 1)
        bait = c.diag(0, 250)
        xb = c.x[bait]
        c.at = xb + 3000
        for k in range(d):
            if k == 0:
                c.diag(0, 200)
            elif k % 61 == 30:
                c.diag(300, 3)
            else:
                c.filler()
        t = c.diag(0, 15, x=max(xb + 5001, c.at))
    assert t == i
    c.diag(0, 15)
    c.filler(2)
    # the last chunk of T's look-back where it depends on the ring: (tier, valid lanes, lane 63 is st)
    last = {(0, ring - 1): ("ring", 63, False), (0, ring): ("ring", 64, True), (0, ring + 1): ("global", 1, False),
            (0, ring + 63): ("global", 63, False), (0, ring + 64): ("global", 64, True), (0, ring + 65): ("global", 1, False),
            (63, ring - 1): ("ring", 63, False), (63, ring): ("ring", 64, True), (63, ring + 1): ("ring_tail", 1, False),
            (63, ring + 63): ("ring_tail", 63, False), (63, ring + 64): ("straddle", 64, True),
            (63, ring + 65): ("global", 1, False)}.get((lane, d))

    def claim(case, ring_, res):
        if ring_ != ring:
            return
        score, parent, facts, jobs = res[0], res[1], res[5], res[6]
        j0 = max(s for s, _, _ in jobs if s <= t)
        assert (t - j0) % 64 == lane, (t, j0)
        rs = recs_of(facts, t)
        assert sum(r["nvalid"] for r in rs) == d
        if d:
            assert parent[t] == t - d and parent[t - d] == bait and score[t] == 15 + 200 + 250, (parent[t], score[t])
            assert rs[-1]["nvalid"] == (d - 1) % 64 + 1 and rs[0]["tier"] == "window"
            assert all(r["tier"] == "ring" for r in rs[1:]) or d > ring - 64
        else:
            assert parent[t] == -1 and (j0 == t) == (lane == 0)
        if last:
            assert (rs[-1]["tier"], rs[-1]["nvalid"], rs[-1]["st_lane63"]) == last, (rs[-1], last)
            if last == ("ring", 64, True) and lane == 0:
                assert t - j0 - d == rs[-1]["live0"]          # the chunk's last ring lane is live0
    return Case("lookback_d%d_l%d_r%d" % (d, lane, ring), *c.arrays(), HDR, claim, rings=(ring,))


def lookback_cases():
    out, seen = [], set()
    for ring in CR.RINGS:
        for d in lookback_d(ring):
            for lane in (0, 63):
                key = (d, lane) if d < 200 else (d, lane, ring)
                if key not in seen:
                    seen.add(key)
                    out.append(lookback_case(d, lane, ring))
    return out


# ------------------------------------------------------------------------------------------------ scripted look-backs
BW_S = 110                         # a bait2 is 103 off T's diagonal
HDR_S = (np.float32(15.0), 5000, 5000, BW_S, 1)
O_RUN, O_BAIT = 100, -100          # a run member and a bait do not see each other (dd = 200 > bw), T sees both (dd = 100)


def scripted(name, roles, claim, lane=10, t_span=15, rings=CR.RINGS, hdr=HDR_S, tail=2):
    """T with the predecessors `roles`: {pos: ("run", span) | ("bait", span) | ("bait2", span) | ("fan", k, span) |
    ("fanbait", span)}, fillers elsewhere, T at lane `lane` of its block.  run: diagonal O_RUN, a member chains onto the
    next one behind it (3 a step), also across fillers.  bait: diagonal O_BAIT, too far off the runs' diagonal to chain
    onto a member.  bait2: directly behind a bait with the same query position (the bait skips it by dq == 0), for a higher
    score behind it.  fan k: diagonal 500 - 10 k (bw 500 cases): the two members of one k chain, members of different k
    skip each other when the farther one has the larger k (dq <= 0).  fanbait: the bait of the fan cases."""
    far = max(roles) + 1
    i = -(-(far + 1 - lane) // 64) * 64 + lane
    c = Call()
    x_t = X0 + DX * i
    for idx in range(i):
        pos = i - 1 - idx
        r = roles.get(pos)
        if r is None:
            c.filler()
        elif r[0] == "run":
            c.diag(O_RUN, r[1])
        elif r[0] == "bait":
            c.diag(O_BAIT, r[1])
        elif r[0] == "bait2":
            c.diag(q=QN + (x_t - DX * pos - X0) - O_BAIT, span=r[1])     # the query position of the bait at pos - 1
        elif r[0] == "fan":
            c.diag(500 - 10 * r[1], r[2])
        elif r[0] == "fanbait":
            c.diag(-300, r[1])                   # 510 and more off every fan diagonal, 300 off T's
    t = c.diag(0, t_span)
    assert t == i and c.x[t] == x_t
    c.filler(tail)

    def wrapped(case, ring, res):
        one_narrow_job(res, len(c.x))
        claim(case, ring, res, t, recs_of(res[5], t))
    return Case(name, *c.arrays(), hdr, wrapped, rings=rings)


def run(near, n, span=15):
    return {p: ("run", span) for p in range(near, near + n)}


def break_case(name, pb, ring, tier, bait=False, behind=13):
    """The 26th bump of T at position pb: a run whose nearest member (pb - 26) improves and whose next 26 are bumps, marked
    by the member in front of each.  behind: members behind the breaking lane (they would mark their parents with T); bait:
    an anchor directly behind the breaking lane that would improve."""
    roles = run(pb - 26, 27)
    nxt = pb + 1
    if bait:
        roles[nxt] = ("bait", 255)
        nxt += 1
    roles.update(run(nxt, behind))

    def claim(case, ring_, res, t, rs):
        if ring_ != ring and tier not in ("window", "ring"):
            return
        target, pairs = res[2], res[4]
        r = rs[-1]
        assert (r["c"], r["brk"], r["tier"]) == (pb // 64, pb % 64, tier), r
        assert r["brk_improver"] == bait and res[1][t] == t - 1 - (pb - 26)
        # the members behind the break in its chunk, but for the run's last one, have a parent to mark
        same_chunk_behind = sum(1 for p in range(nxt, nxt + behind - 1) if p // 64 == pb // 64)
        assert len(r["brk_marks"]) == same_chunk_behind
        if same_chunk_behind:
            assert any(target[p] != t for p in r["brk_marks"])            # marks behind the break would change targets
        assert len(rs) == pb // 64 + 1 and sum(len(q["hits"]) for q in rs) == 26
        assert all(h[1] == "same" for h in rs[-1]["hits"][1:])
    return scripted(name, roles, claim, rings=(ring,) if tier not in ("window", "ring") else CR.RINGS)


def break_cases():
    out = [break_case("break_window_mid_bait", 40, 512, "window", bait=True),
           break_case("break_window_l63", 63, 512, "window"),
           break_case("break_ring_l0_bait", 64, 512, "ring", bait=True),
           break_case("break_ring_mid", 64 + 30, 512, "ring")]
    for R in CR.RINGS:
        # T at lane 10: chunk R/64 holds the anchors [live0 - 54, live0 + 9], lanes 0..9 in the ring, 10..63 in global memory
        out += [break_case("break_straddle_ringpart_r%d" % R, R + 5, R, "straddle"),
                break_case("break_straddle_mid_bait_r%d" % R, R + 30, R, "straddle", bait=True),
                break_case("break_straddle_l63_r%d" % R, R + 63, R, "straddle"),
                break_case("break_global_l0_r%d" % R, R + 64, R, "global"),
                break_case("break_global_mid_bait_r%d" % R, R + 64 + 30, R, "global", bait=True),
                break_case("break_global_l63_r%d" % R, R + 127, R, "global")]
    return out


# ------------------------------------------------------------------------------------------------ phase-3 shapes
def shape_cases():
    out = []

    def shapes(rs):
        return [(r["c"], r["shape"]) for r in rs if r["nopen"]]          # chunks of fillers alone are left out

    def quiet(case, ring, res, t, rs):
        # two lone anchors that cannot beat T's own span: an open lane in the window and one in chunk 1, nothing happens
        assert shapes(rs) == [(0, "quiet"), (1, "quiet")] and res[1][t] == -1
        assert [(r["nopen"], len(r["marks"])) for r in rs] == [(1, 0), (1, 0)]
    out.append(scripted("shape_quiet", {5: ("run", 1), 70: ("bait", 1)}, quiet, t_span=255, tail=2))

    def by_c(rs):
        return {r["c"]: r for r in rs}

    # every case but the quiet one ends in a break, so that the n_skip its chunks hand on shows in the outputs
    def popcount(case, ring, res, t, rs):
        # T's span 255 beats every candidate: 15 bumps and no improver in the window, the 26th in chunk 1 at lane 10
        assert shapes(rs) == [(0, "popcount"), (1, "popcount")] and res[1][t] == -1
        assert len(rs[0]["hits"]) == 15 and (rs[1]["nskip_in"], rs[1]["brk"]) == (15, 10)
    roles = run(0, 16)
    roles.update(run(64, 14))
    out.append(scripted("shape_popcount", roles, popcount, t_span=255))

    def lead(case, ring, res, t, rs):
        # the nearest run member improves, the other 9 are bumps (window); in chunk 2 a bait improves (n_skip 9 -> 8), a
        # lower one behind it does nothing; the run goes on in chunk 3 and its 18th member there is the 26th bump
        r = by_c(rs)
        assert shapes(rs) == [(0, "lead"), (2, "lead"), (3, "popcount")], shapes(rs)
        assert (r[2]["nskip_in"], r[2]["dec"], r[3]["nskip_in"], r[3]["brk"]) == (9, 1, 8, 17) and res[1][t] == t - 1 - 130
    roles = run(3, 10)
    roles[130] = ("bait", 200)
    roles[131] = ("bait", 100)
    roles.update(run(192, 30))
    out.append(scripted("shape_lead", roles, lead))

    def scan(case, ring, res, t, rs):
        # improver, 9 bumps, then a bait on the other side of T's diagonal behind them: the walk starts with -1 and is
        # reflected, n_skip leaves the window as 8; the run goes on in chunk 1, its 18th member there breaks
        r = by_c(rs)
        assert shapes(rs) == [(0, "scan"), (1, "popcount")] and r[0]["walk_neg"] and r[0]["dec"] == 1 and res[1][t] == t - 1 - 45
        assert len(r[0]["hits"]) == 9 and (r[1]["nskip_in"], r[1]["brk"]) == (8, 17)
    roles = run(2, 10)
    roles[45] = ("bait", 255)
    roles.update(run(64, 30))
    out.append(scripted("shape_scan_window_reflect", roles, scan))

    def scan_later(case, ring, res, t, rs):
        r = by_c(rs)
        assert shapes(rs) == [(2, "scan"), (3, "popcount")] and r[2]["walk_neg"] and res[1][t] == t - 1 - 180
        assert (r[3]["nskip_in"], r[3]["brk"]) == (8, 17)
    roles = run(130, 10)
    roles[180] = ("bait", 255)
    roles.update(run(192, 30))
    out.append(scripted("shape_scan_later_reflect", roles, scan_later))

    def carried(case, ring, res, t, rs):
        # 15 bumps in the window (T's span 255 beats the run), 6 more in chunk 1 and then two improvers: n_skip 21 -> 19,
        # the walk never below 0; in chunk 2 the run goes on: 7 more bumps break at 26 - two lanes later than without
        # the improvers
        assert shapes(rs) == [(0, "popcount"), (1, "scan"), (2, "popcount")], shapes(rs)
        assert rs[1]["nskip_in"] == 15 and rs[1]["dec"] == 2 and not rs[1]["walk_neg"]
        assert rs[2]["nskip_in"] == 19 and rs[2]["brk"] == 6 and res[1][t] == t - 1 - 101
    roles = run(0, 16)
    roles.update(run(64, 6))
    roles[100] = ("bait", 200)
    roles[101] = ("bait2", 255)
    roles.update(run(128, 12))
    out.append(scripted("shape_carried_nskip", roles, carried, t_span=255))
    return out


# ------------------------------------------------------------------------------------------------ marks
HDR_F = (np.float32(15.0), 5000, 5000, 500, 1)


def fan_case(name, far, ring, nfan, bait_pos, claim_more):
    """Two interleaved sets of diagonals: near anchors N_k at pos k and far anchors F_k at pos far + k, k = 0 .. nfan-1, a pair
    per diagonal.  The N_k skip each other and so do the F_k (dq <= 0), N_k's parent is F_k.  T improves on none of them:
    in the window it marks every F_k, `far` lanes on every F_k is a bump.  A bait behind them would improve."""
    roles = {k: ("fan", k, 15) for k in range(nfan)}
    roles.update({far + k: ("fan", k, 15) for k in range(nfan)})
    assert bait_pos not in roles
    roles[bait_pos] = ("fanbait", 255)

    def claim(case, ring_, res, t, rs):
        if ring_ != ring:
            return
        parent = res[1]
        assert all(parent[t - 1 - k] == t - 1 - far - k for k in range(nfan))
        assert [m[1] for m in rs[0]["marks"]] == [t - 1 - far - k for k in range(nfan)] and rs[0]["shape"] == "quiet"
        claim_more(res, t, [r for r in rs if r["nopen"]])
    return scripted(name, roles, claim, rings=(ring,), hdr=HDR_F)


def mark_cases():
    out = []
    for R in CR.RINGS:
        def straddle(res, t, rs, R=R):
            # T at lane 10: live0 = t - 10 - R.  F_14 is anchor live0 (marked in the ring), F_15 is live0 - 1 (direct store),
            # F_4 is one full ring behind T.  Chunk R/64 - 1 sees F_0..F_4, chunk R/64 the rest: lanes 0..9 learn their mark
            # from the ring, lanes 10.. from global memory; the 26th bump, F_25 at lane 20, breaks in front of the bait.
            live0 = t - 10 - R
            marks = {m[1]: m[2] for m in rs[0]["marks"]}
            assert marks[live0] == "ring" and marks[live0 - 1] == "direct" and marks[t - R] == "ring" and rs[0]["live0"] == live0
            last = rs[-1]
            assert (last["tier"], last["brk"], last["c"]) == ("straddle", 20, R // 64) and last["brk_improver"]
            assert [h[1] for h in last["hits"]] == ["ring"] * 10 + ["global"] * 11
            assert [h[1] for h in rs[-2]["hits"]] == ["ring"] * 5 and res[1][t] == -1
        out.append(fan_case("marks_straddle_r%d" % R, R - 5, R, 30, R + 26, straddle))

        def glob(res, t, rs, R=R):
            # every F_k has left the ring: 30 direct stores in the window chunk, 26 hits through global memory
            assert all(m[2] == "direct" for m in rs[0]["marks"]) and len(rs[0]["marks"]) == 30
            last = rs[-1]
            assert (last["tier"], last["brk"]) == ("global", 35) and last["brk_improver"]
            assert [h[1] for h in last["hits"]] == ["global"] * 26
        out.append(fan_case("marks_global_r%d" % R, R + 64 + 10, R, 30, R + 64 + 42, glob))

        def glob_nobreak(res, t, rs, R=R):
            # 20 bumps through global memory, then the bait improves: a scan in a global chunk, n_skip 20 -> 19
            last = rs[-1]
            assert (last["tier"], last["brk"], last["shape"], last["dec"]) == ("global", None, "scan", 1)
            assert res[1][t] == t - 1 - (R + 64 + 40)
        out.append(fan_case("marks_global_scan_r%d" % R, R + 64 + 10, R, 20, R + 64 + 40, glob_nobreak))

    def ring_hits(res, t, rs):
        last = rs[-1]
        assert (last["tier"], last["brk"]) == ("ring", 100 + 25 - 64) and [h[1] for h in last["hits"]] == ["ring"] * 26
    out.append(scripted_fan_ring(ring_hits))
    return out


def scripted_fan_ring(claim_more):
    roles = {k: ("fan", k, 15) for k in range(30)}
    roles.update({100 + k: ("fan", k, 15) for k in range(30)})
    roles[140] = ("fanbait", 255)

    def claim(case, ring, res, t, rs):
        assert all(m[2] == "ring" for m in rs[0]["marks"])
        claim_more(res, t, [r for r in rs if r["nopen"]])
    return scripted("marks_ring", roles, claim, hdr=HDR_F)


# ------------------------------------------------------------------------------------------------ narrow-path folds
def probes_call(name, hdr, probes, q0=500, x0=X0, spans=(15, 0, 255, 7), segs=None, claim=None, gap=None):
    """Isolated anchor pairs: the second anchor of pair k lies (dr, dq) past the first, whose span is above every gap cost
    used here, so the second chains iff the pair is not skipped.  Pairs are farther apart than max_dist_x: no anchor sees
    another pair (and the first pair boundary of a block of 64 is a cut)."""
    c = Call(x0=x0)
    mdx = int(hdr[1])
    gap = gap if gap is not None else max(mdx, 0) + 1000
    x = x0
    for k, (dr, dq) in enumerate(probes):
        a = c._put(q0 + 40 * k, (200, 255)[k % 2], 0, x)        # above every gap cost here: b chains iff it is not skipped
        b = c._put(q0 + 40 * k + dq, spans[k % len(spans)], 0 if segs is None else segs[k % len(segs)], x + dr)
        assert b == a + 1
        x += dr + gap

    def base_claim(case, ring, res):
        assert all(nar for _, _, nar in res[6]) == (segs is None), res[6]
        if claim:
            claim(case, ring, res)
    return Case(name, *c.arrays(), hdr, base_claim)


def fold_cases():
    out = []
    small = [(1, 1), (5, 5), (0, 5), (5, 0), (7, 3), (3, 7), (0, 0), (40, 39)]

    def chained(want):
        def claim(case, ring, res):
            got = [int(p) >= 0 for p in res[1][1::2]]
            assert got == want, (case.name, got, want)
        return claim
    # dq == min(max_dist_x, max_dist_y) and one more, each of the two being the smaller
    for nm, mdx, mdy in (("x", 800, 5000), ("y", 5000, 800)):
        pr = [(799, 799), (800, 800), (801, 801), (300, 800), (300, 801), (300, 799)]
        want = [True, True, False, True, False, True]
        out.append(probes_call("fold_dq_lim_%s" % nm, (np.float32(15.0), mdx, mdy, 600, 1), pr, claim=chained(want), gap=9000))
    for ns in (1, 2):
        for mdy in (0, -5):
            out.append(probes_call("fold_mdy%d_segs%d" % (mdy, ns), (np.float32(15.0), 5000, mdy, 500, ns), small,
                                   claim=chained([False] * len(small))))
    out.append(probes_call("fold_mdx0", (np.float32(15.0), 0, 5000, 500, 1), small, claim=chained([False] * len(small))))
    bwp = [(100, 100), (101, 100), (100, 101), (100, 99), (0, 5), (250, 250)]
    out.append(probes_call("fold_bw0", (np.float32(15.0), 5000, 5000, 0, 1), bwp, claim=chained([True, False, False, False, False, True])))
    out.append(probes_call("fold_bw_neg", (np.float32(15.0), 5000, 5000, -1, 1), bwp, claim=chained([False] * 6)))
    bwe = [(130, 100), (131, 100), (100, 130), (100, 131)]
    out.append(probes_call("fold_bw30", (np.float32(15.0), 5000, 5000, 30, 1), bwe, claim=chained([True, False, True, False])))
    # n_segs 2: dr == max_dist_y and one more (dq far below it)
    drp = [(800, 700), (801, 700), (799, 700), (800, 800), (801, 800)]
    out.append(probes_call("fold_dr_lim_segs2", (np.float32(15.0), 5000, 800, 500, 2), drp, claim=chained([True, False, True, True, False])))
    out.append(probes_call("fold_dr_lim_segs1", (np.float32(15.0), 5000, 800, 500, 1), drp, claim=chained([True, True, True, True, True])))
    # dr == 0 duplicates, three deep, then a proper successor
    c = Call()
    for k in range(6):
        c._put(500 + 10 * k, 15, 0, X0 + 30 * (k // 3))

    def dup(case, ring, res):
        one_narrow_job(res, 6)
        parent = [int(p) for p in res[1]]
        assert parent[:3] == [-1, -1, -1] and all(p in (0, 1, 2) for p in parent[3:]), parent
        assert sum(r["nopen"] for r in res[5]) == 9           # 3 x 3 pairs across the two positions, none inside one
    out.append(Case("fold_dr0_duplicates", *c.arrays(), HDR, dup))
    # query words with bit 31 set: (int)y negative, and a pair across 2^32 (-16 -> 5); differences stay small
    out.append(probes_call("fold_q_bit31", HDR, small + [(100, 100), (90, 100)], q0=0x80000010, claim=chained(
        [True, True, False, False, True, True, False, True, True, True])))
    out.append(probes_call("fold_q_wrap32", HDR, [(21, 21), (30, 21)], q0=0xfffffff0 - 40, claim=chained([True, True])))
    # low x words just below 2^32 under an upper word with the strand bit
    top = (1 << 63) | (5 << 32)
    out.append(probes_call("fold_x_top", HDR, [(5, 5), (100, 90), (0, 3), (50, 60)], x0=top | (0xffffffff - 4 * 6200),
                           claim=chained([True, True, False, True])))
    return out


def upper_word_case():
    """40 anchors up to (5 << 32) | 0xfffffffd, 40 more from (6 << 32) | 0x10 on, one diagonal: the 64-bit dr across the
    boundary is small, so there is no cut and the job is not narrow; the chain runs across."""
    c = Call(x0=(5 << 32) | (0x100000000 - 3 * 40))
    for k in range(40):
        c.diag(0, 15)
    assert c.x[-1] >> 32 == 5 and c.at >> 32 == 6
    c.at = (6 << 32) | 0x10
    for k in range(40):
        c.diag(0, 15)

    def claim(case, ring, res):
        assert res[6] == [(0, 80, False)]
        assert res[1][40] == 39 and res[0][79] > res[0][39] > 15 * 5
    return Case("upper_word_in_reach", *c.arrays(), HDR, claim)


# ------------------------------------------------------------------------------------------------ fp64 gap cost
QSPANS = (100.0, 50.0, 12.5, 14.2857, 0.0, 1e6)


def gap_case(aq):
    """dd = 1 .. bw (120) on a pair each: c_lin = (int)(dd * .01 * avg_qspan) in fp64, in the reference's order of
    multiplications (29 * .01 * 100.0 is 28.999...)."""
    hdr = (np.float32(aq), 5000, 5000, 120, 1)
    pr = [(200 + dd, 200) for dd in range(1, 121)]

    def claim(case, ring, res):
        score = res[0][1::2].astype(np.int64)
        dd = np.arange(1, 121)
        c_lin = np.trunc(dd * .01 * float(np.float32(aq))).astype(np.int64)
        assert aq != 100.0 or (c_lin[28], c_lin[29]) == (28, 30)
        log2 = np.floor(np.log2(dd)).astype(np.int64)
        span = (case.y >> np.uint64(32) & np.uint64(0xff)).astype(np.int64)
        first, spans = span[0::2], span[1::2]
        want = np.minimum(200, spans) - (c_lin + (log2 >> 1)) + first
        chained = want > spans
        assert np.array_equal(score[chained], want[chained]) and np.array_equal(score[~chained], spans[~chained])
        assert chained.sum() == (120 if aq < 1e5 else 0)      # at 1e6 every c_lin is 10 000 and more: nobody chains
    return probes_call("gap_aq%g" % aq, hdr, pr, claim=claim, gap=6000)


# ------------------------------------------------------------------------------------------------ unsorted
def pair_dd(x, y, i, j):
    """(dd, same) of the pair as host_kernel.cpp:59-64 computes them"""
    dr = (int(x[i]) - int(x[j])) & CR.M64
    dr = dr - (1 << 64) if dr >> 63 else dr
    dq = int(CR._wrap32((int(y[i]) & 0xffffffff) - (int(y[j]) & 0xffffffff)))
    dd = int(CR._wrap32(dr - dq if dr > dq else dq - dr))
    return dd, (int(y[i]) >> 48 & 0xff) == (int(y[j]) >> 48 & 0xff)


def unsorted_two():
    x = np.array([(1 << 32) | 900, 1000], dtype=np.uint64)
    y = np.array([(0 << 48) | (15 << 32) | 50, (1 << 48) | (15 << 32) | 70], dtype=np.uint64)

    def claim(case, ring, res):
        assert [list(a) for a in res[:4]] == [[15, 41], [-1, 0], [0, 0], [15, 41]] and res[4] == 1
        assert res[6] == [(0, 2, False)] and pair_dd(x, y, 1, 0) == (-80, False)
    return Case("unsorted_two", x, y, (np.float32(15.0), 5000, 800, 500, 2), claim)


def unsorted_300(seed=11):
    """300 anchors, upper x words 1 and 0 in alternating runs of 10 (not sorted), segment ids 0, 1, 2 in runs of 45.  Where
    an anchor of word 0 looks back at one of word 1 the 64-bit dr has wrapped, and dd = (int32)(dq - dr) is negative when
    the low words differ by more than dq: the low words rise by 15 an anchor, the query by 5.  At the head of a word 0 run
    those are the nearest candidates."""
    rng = np.random.default_rng(seed)
    low = 2000 + np.cumsum(rng.integers(5, 25, 300))
    q = 300 + np.cumsum(rng.integers(1, 9, 300))
    up = (1 - (np.arange(300) // 10) % 2).astype(np.uint64)
    seg = ((np.arange(300) // 45) % 3).astype(np.uint64)
    x = (up << np.uint64(32)) | low.astype(np.uint64)
    y = (seg << np.uint64(48)) | (np.uint64(15) << np.uint64(32)) | q.astype(np.uint64)

    def claim(case, ring, res):
        parent = res[1]
        assert res[6] == [(0, 300, False)]
        links = [pair_dd(x, y, i, int(parent[i])) for i in range(300) if parent[i] >= 0]
        # chains pass through both kinds; with the same segment id the gap cost is negative from dd = -107 on
        # ((int)(dd * .15) + (31 >> 1) < 0), with different ones at once (min(c_lin, 31))
        neg_same = sum(1 for dd, same in links if dd <= -107 and same)
        neg_diff = sum(1 for dd, same in links if dd <= -7 and not same)
        assert neg_same >= 3 and neg_diff >= 3, (neg_same, neg_diff)
    return Case("unsorted_300", x, y, (np.float32(15.0), 5000, 800, 500, 3), claim)


# ------------------------------------------------------------------------------------------------ cuts
def clusters_call(name, sizes, keys, claim):
    """clusters of diagonal anchors 7000 reference bases apart; keys[k]: x of the cluster's first anchor (64 bits)"""
    c = Call()
    for size, key in zip(sizes, keys):
        c.at = key
        for _ in range(size):
            c.diag(0, 15)
    return Case(name, *c.arrays(), HDR, claim)


def cut_cases():
    out = []
    lo = 0x100000000

    def jobs_are(want):
        def claim(case, ring, res):
            assert res[6] == want, res[6]
        return claim
    # cuts at lane 0 (anchor 64) and lane 63 (anchor 191) of their blocks, and at lane 2 (194); a second cut of that
    # block (anchor 224) is not taken
    out.append(clusters_call("cut_lane0_lane63", [64, 127, 3, 30, 10], [1000, 9000, 17000, 25000, 33000],
                             jobs_are([(0, 64, True), (64, 127, True), (191, 3, True), (194, 40, True)])))
    # upper words differ only before the cut / only after it / on both sides (each time across a word boundary within reach)
    b5, b6 = (5 << 32) + lo - 60, (6 << 32) + lo - 60
    out.append(clusters_call("cut_words_before", [40, 40], [b5, (6 << 32) | 20000], jobs_are([(0, 40, False), (40, 40, True)])))
    out.append(clusters_call("cut_words_after", [40, 40], [(5 << 32) | 0xfff00000, b5], jobs_are([(0, 40, True), (40, 40, False)])))
    out.append(clusters_call("cut_words_both", [40, 40], [b5, b6], jobs_are([(0, 40, False), (40, 40, False)])))
    return out


def neighbours():
    """a sorted call on either side of the unsorted one, both cut"""
    def jobs_are(want):
        def claim(case, ring, res):
            assert res[6] == want, res[6]
        return claim
    # (the cut at anchor 30 takes block 0's one cut; 80 is the first of block 1)
    a = clusters_call("sorted_before_unsorted", [30, 50, 10], [1000, 9000, 17000], jobs_are([(0, 30, True), (30, 50, True), (80, 10, True)]))
    b = clusters_call("sorted_after_unsorted", [70, 70], [1000, 9000], jobs_are([(0, 70, True), (70, 70, True)]))
    return a, b


def maxiter_case():
    """5002 fillers one base apart under max_dist_x 100000: anchors 5000 and 5001 look back at exactly max_iter anchors"""
    c = Call(dx=1)
    c.filler(5002)

    def claim(case, ring, res):
        one_narrow_job(res, 5002)
        assert res[4] == sum(min(i, 5000) for i in range(5002))
        assert sum(r["nvalid"] for r in recs_of(res[5], 5001)) == 5000
    return Case("max_iter", *c.arrays(), (np.float32(15.0), 100000, 100000, 500, 1), claim)


# ------------------------------------------------------------------------------------------------ families
def families():
    """name -> [Case].  The device test runs a family as one call list."""
    if "families" not in _cache:
        a, b = neighbours()
        _cache["families"] = {
            "lengths": [length_case(n) for n in LENGTHS],
            "lookback": lookback_cases(),
            "breaks": break_cases(),
            "shapes": shape_cases(),
            "marks": mark_cases(),
            "folds": fold_cases(),
            "upper_word": [upper_word_case()],
            "gap": [gap_case(aq) for aq in QSPANS],
            "unsorted": [a, unsorted_two(), unsorted_300(), b],
            "cuts": cut_cases(),
            "max_iter": [maxiter_case()],
        }
    return _cache["families"]


NARROW_OR_CUT = ("lengths", "lookback", "breaks", "shapes", "marks", "folds", "gap", "cuts", "unsorted", "max_iter")


def pack(cases):
    from cases import chain_pack
    return chain_pack([c.call for c in cases])
