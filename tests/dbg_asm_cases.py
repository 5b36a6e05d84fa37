"""Hand-built dbg_asm calls at the edges of csrc/dbg_asm_kernels.hip and of the retry in csrc/capi_dbg_asm.hip: cycles of
every small shape and the edges the cycle check leaves out, node counts around the wavefront width and the LDS-to-workspace
switch, many sources at once, homopolymer runs that stop looping at a chosen k, bubbles of every kind, branchings that end
on either side of the give-up limits, long paths and many starts.  Builders only (dbg_cases.py's Case, no GPU): every case
carries a check that asserts on the restatement (tests/dbg_asm_ref.py) that it is what its name says;
tests/test_dbg_asm_cpu.py calls the checks, tests/test_dbg_asm_gpu.py runs the cases on the device.

Not built: a path whose last node is REF only.  A search extends READ-only nodes alone, an edge out of one comes from a read,
and a read colours both its nodes READ: no graph of the builder has such an edge (the reference's own comment at that
branch: "Not quite sure how this could happen")."""
import os

import numpy as np

import dbg_asm_ref as AR
import dbg_cases as DC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LDS_NODES = 4096                         # DBG_ASM_LDS_NODES: in-degrees and list in LDS up to this many nodes
WAVE = 64
REFSYM = bytes(b for b in range(48, 91) if chr(b).isalnum() and chr(b) not in "NA")    # digits and capitals but N and A
PAD = b"~"                               # a read's last base is in no occurrence (i runs to l_seq - k - 2)
POS = 1000


def uniq(rng, n, k, seen=None):
    """n bytes over REFSYM whose k-mers are all different (and not in `seen`, which they join)"""
    seen = set() if seen is None else seen
    out = bytearray()
    while len(out) < n:
        for _ in range(64):
            c = REFSYM[int(rng.integers(len(REFSYM)))]
            km = bytes(out[len(out) - k + 1:]) + bytes([c]) if len(out) >= k - 1 else None
            if km is None or km not in seen:
                break
        else:
            raise RuntimeError("no free k-mer")
        if km is not None:
            seen.add(km)
        out.append(c)
    return bytes(out)


def rd(seq, q=40, flag=0):
    return DC.read(seq + PAD, q, flag)


class AsmCase(DC.Case):
    """A dbg call with its assembly params (ap: keyword overrides of dbg_asm_ref.DEFAULTS)"""

    def __init__(self, name, k, reads, wins, check=None, min_qual=20, ap=None, **facts):
        super().__init__(name, k, min_qual, reads, wins, check, **facts)
        self.ap = AR.params(**(ap or {}))
        self._asm = None

    def want_asm(self):
        if self._asm is None:
            self._asm = [AR.window(ref, pos, self.reads[lo:hi], self.k, self.min_qual, self.ap) for ref, pos, lo, hi in self.wins]
        return self._asm

    def asm_params(self):
        from genomicsbench_amd import dbg_asm as A
        return A.make_asm_params(**self.ap)


NO_RETRY = dict(k_last=0)


def one(name, k, ref, reads=(), check=None, **kw):
    reads = list(reads)
    return AsmCase(name, k, reads, [(ref, POS, 0, len(reads))], check, **kw)


def join(name, cases, check=None, ap=None, **facts):
    reads, wins = [], []
    for c in cases:
        assert (c.k, c.min_qual) == (cases[0].k, cases[0].min_qual)
        wins += [(ref, pos, lo + len(reads), hi + len(reads)) for ref, pos, lo, hi in c.wins]
        reads += c.reads
    return AsmCase(name, cases[0].k, reads, wins, check, cases[0].min_qual, ap if ap is not None else {f: cases[0].ap[f] for f in AR.DEFAULTS},
                   parts=cases, **facts)



def expect(**want):
    """a check: every window's fields (or, for a list, the windows' values in order)"""
    def check(case):
        ws = case.want_asm()
        for f, v in want.items():
            got = [len(w["starts"]) if f == "n_starts" else w["stats"]["n_nodes"] if f == "n_nodes" else w[f] for w in ws]
            assert got == (list(v) if isinstance(v, (list, tuple)) else [v] * len(ws)), (case.name, f, got, v)
    return check


# ------------------------------------------------------------------------------------------------- cycles
def fit_nodes(make, n):
    """make(length) -> case of one window; the length at which its graph has n nodes"""
    L = n
    for _ in range(4):
        c = make(L)
        have = c.want()[0][0]["n_nodes"]
        if have == n:
            return c
        L += n - have
    raise AssertionError("no length gives %d nodes" % n)


def line_case(name, n, k=5, tail=b"", seed=1, cyclic=0):
    """a line of n nodes; tail b"xyxyxyxy": a 2-cycle behind it"""
    def make(L):
        return one(name, k, uniq(np.random.default_rng(seed), L, k) + tail, check=expect(cyclic=cyclic, n_nodes=n), ap=NO_RETRY)
    return fit_nodes(make, n)


def jump_back(q, into_ref, k=3):
    """A line of reference and one read that leaves it at its 20th base for the 6th: through READ-only junction nodes (weight
    q on the edge into the first), or with into_ref straight into a reference k-mer upstream (the reference is spelled so that
    the read's k + 1 bases are k-mer 17 and then k-mer 5)."""
    rng = np.random.default_rng(7)
    ref = bytearray(uniq(rng, 30, k))
    if into_ref:
        ref[18:20] = ref[5:7]                                # k-mer [17, 20) ends in the 2 bases k-mer [5, 8) starts with
        read = bytes(ref[17:20]) + bytes(ref[7:8])
    else:
        read = bytes(ref[10:20]) + bytes(ref[5:15])
    return bytes(ref), rd(read, q)


def cycle_cases():
    out = [one("self_loop", 3, b"AAAAAA", check=expect(cyclic=1, n_nodes=1), ap=NO_RETRY),
           one("two_cycle", 3, b"BCBCBCB", check=expect(cyclic=1, n_nodes=2), ap=NO_RETRY)]
    rng = np.random.default_rng(3)
    u = uniq(rng, 40, 5)
    out.append(one("long_cycle", 5, u[:30] + u[5:10] + u[30:], check=expect(cyclic=1), ap=NO_RETRY))          # k-mer [5, 10) twice: a ring of 25
    out.append(one("diamond", 5, u, [rd(u[8:15] + b"a" + u[16:23])], check=expect(cyclic=0, n_starts=1, n_paths=1), ap=NO_RETRY))
    for q, cyc in ((39, 0), (40, 1)):
        ref, read = jump_back(q, False)
        out.append(one("closing_read_edge_%d" % q, 3, ref, [read], check=expect(cyclic=cyc), ap=NO_RETRY))
    ref, read = jump_back(1, True)
    out.append(one("closing_edge_into_ref_weight_1", 3, ref, [read], check=expect(cyclic=1), min_qual=1, ap=NO_RETRY))
    # the closing edge as the fifth successor of its node: dropped, acyclic; the same reads with it first: cyclic
    sibs = [rd(ref[17:20] + bytes([c]), 1) for c in b"abc"]
    out.append(one("closing_edge_dropped", 3, ref, sibs + [read], check=expect(cyclic=0), min_qual=1, ap=NO_RETRY))
    out.append(one("closing_edge_kept", 3, ref, [read] + sibs, check=expect(cyclic=1), min_qual=1, ap=NO_RETRY))
    for n in (WAVE - 1, WAVE, WAVE + 1):
        out.append(line_case("line_%d" % n, n))
        out.append(line_case("line_%d_cycle" % n, n, tail=b"xyxyxyxy", cyclic=1))
    for n in (LDS_NODES - 1, LDS_NODES, LDS_NODES + 1):
        out.append(line_case("line_%d" % n, n, seed=n))
        out.append(line_case("line_%d_cycle" % n, n, tail=b"xyxyxyxy", seed=n, cyclic=1))
    # nothing but a ring: the last k-mer leads back into the first.  64 and 4096: powers of two, where the kernel's in-place
    # pointer jumping can leave ring nodes pointing at themselves (and the wavefront width and the LDS limit)
    for n in (40, WAVE, LDS_NODES, LDS_NODES + 904):
        u = uniq(np.random.default_rng(n), n, 5)
        out.append(one("ring_%d" % n, 5, u + u[:6], check=expect(cyclic=1, n_nodes=n), ap=NO_RETRY))
    for n in (WAVE + 6, 4 * WAVE + 44):                      # that many sources at once: disjoint pairs of read k-mers
        seen = set()
        rng = np.random.default_rng(n)
        ref = uniq(rng, 20, 5, seen)
        pairs = [rd(uniq(rng, 6, 5, seen)) for _ in range(n)]
        out.append(one("sources_%d" % n, 5, ref, pairs, check=expect(cyclic=0, n_nodes=15 + 2 * n), ap=NO_RETRY))
        out.append(one("sources_%d_cycle" % n, 5, ref + b"xyxyxyxy", pairs, check=expect(cyclic=1), ap=NO_RETRY))
    by = {c.name: c for c in out}
    empty = AsmCase("empty", 5, [], [(b"", POS, 0, 0), (b"BCDEFG", POS, 0, 0)], expect(cyclic=0, n_nodes=0), ap=NO_RETRY)
    out.append(empty)
    out.append(join("cyclic_between_acyclic", [by["line_63"], empty, by["line_64_cycle"], by["line_65"], by["long_cycle"], empty, by["diamond"]],
                    expect(cyclic=[0, 0, 0, 1, 0, 1, 0, 0, 0])))
    out.append(join("long_cycle_256_times", [by["long_cycle"]] * 256, expect(cyclic=1)))
    return out


# ------------------------------------------------------------------------------------------------- retry
def run_ref(run, seed=5, flank=70, total=None):
    """unique flanks around a run of 'A' (every k-mer of 15 bases and more is there once, but the run's)"""
    rng = np.random.default_rng(seed)
    u = uniq(rng, 2 * flank, 15)
    ref = u[:flank] + b"A" * run + u[flank:]
    return ref if total is None else ref[flank - 1:flank - 1 + total]


def retry_cases():
    def run(name, n, k, builds, cyc=0, **kw):
        return one(name, 15, run_ref(n), check=expect(k=k, n_builds=builds, cyclic=cyc), **kw)
    out = [run("run_18", 18, 20, 2), run("run_28", 28, 30, 4), run("run_53", 53, 55, 9), run("run_60", 60, 55, 9, cyc=1),
           run("run_18_step_1", 18, 18, 4, ap=dict(k_step=1)), run("run_18_no_retry", 18, 15, 1, cyc=1, ap=dict(k_last=10)),
           run("run_15", 15, 15, 1), run("run_16", 16, 20, 2)]
    # 28 'A' in a reference of 30: cyclic at 15, 20 and 25, and shorter than k + 2 at 30
    out.append(one("ref_runs_out", 15, run_ref(28, total=30), check=expect(k=30, n_builds=4, cyclic=0, n_nodes=0)))
    runs = [18, 23, 28, 33, 38, 43, 48, 53]
    shrink = [one("", 15, run_ref(n, seed=n)) for n in runs]
    ks = [20, 25, 30, 35, 40, 45, 50, 55]
    out.append(join("shrinks_to_last", shrink, expect(k=ks, cyclic=0)))
    out.append(join("shrinks_to_first", shrink[::-1], expect(k=ks[::-1], cyclic=0)))
    return out


# ------------------------------------------------------------------------------------------------- paths
def bubble(ref, x, alt, dele, k, q=40, left=None, right=None):
    """a read that spells ref around x with `dele` bases replaced by alt"""
    left, right = (k + 2 if left is None else left), (k + 2 if right is None else right)
    return rd(ref[x - left:x] + alt + ref[x + dele:x + dele + right], q)


def path_cases():
    out = []
    for k in (3, 15):
        ref = uniq(np.random.default_rng(k), 90, k)
        for name, alt, dele, n_nodes in (("snp", b"a", 1, k + 2), ("insertion", b"abc", 0, k + 4), ("deletion", b"", 3, k + 1)):
            out.append(one("%s_k%d" % (name, k), k, ref, [bubble(ref, 40, alt, dele, k)],
                           check=expect(cyclic=0, n_starts=1, n_paths=1, n_path_nodes=n_nodes), ap=NO_RETRY))
    k = 3
    ref = uniq(np.random.default_rng(11), 60, k)
    out.append(one("start_edge_39", k, ref, [bubble(ref, 30, b"a", 1, k, 39)], check=expect(n_starts=0), ap=NO_RETRY))
    out.append(one("start_edge_40", k, ref, [bubble(ref, 30, b"a", 1, k, 40)], check=expect(n_starts=1, n_paths=1), ap=NO_RETRY))
    # the bubble spells two reference bases (50, 51) in its middle; a weak read leaves it there: into READ-only nodes (not
    # taken), or with the reference's next base straight into the reference's k-mer [50, 53) (taken: a second, shorter path)
    strong = bubble(ref, 30, b"ab" + ref[50:52] + b"cd", 1, k)
    out.append(one("weak_edge_into_read", k, ref, [strong, rd(b"b" + ref[50:52] + b"xyz", 25)], check=expect(n_starts=1, n_paths=1), ap=NO_RETRY))
    out.append(one("weak_edge_into_ref", k, ref, [strong, rd(b"b" + ref[50:53], 25)], check=expect(n_starts=1, n_paths=2), ap=NO_RETRY))
    out.append(one("dead_end", k, ref, [rd(ref[25:30] + b"abcdef")], check=expect(n_starts=1, n_paths=0, n_gave_up=0), ap=NO_RETRY))
    out.append(one("read_self_loop", k, ref, [bubble(ref, 30, b"zzzzzz", 0, k)], check=expect(cyclic=1, n_starts=1, n_paths=1), ap=NO_RETRY))
    out.append(one("read_3_cycle", k, ref, [bubble(ref, 30, b"xyzxyzxyz", 0, k)], check=expect(cyclic=1, n_starts=1, n_paths=1), ap=NO_RETRY))
    for nb in (2, 3, 4):
        reads = [bubble(ref, 30, b"a" + bytes([c]), 2, k) for c in b"bcde"[:nb]]
        out.append(one("branches_%d" % nb, k, ref, reads, check=expect(n_starts=1, n_paths=nb), ap=NO_RETRY))
    combos = [b"a" + bytes([x, y, z]) for x in b"bcde" for y in b"bcde" for z in b"bcde"]
    for n, paths, gave in ((20, 20, 0), (21, 21, 0), (22, 0, 1)):
        reads = [bubble(ref, 30, c, 4, k) for c in combos[:n]]
        out.append(one("finished_%d" % n, k, ref, reads, check=expect(n_starts=1, n_paths=paths, n_gave_up=gave), ap=NO_RETRY))
    for want_peak, max_pending in ((20, 20), (21, 20), (59, 59), (60, 59)):
        # a main read that never returns, behind short reads that give each of its nodes three (the last one perhaps fewer)
        # more successors: three more paths pending per level.  max_pending 59 is the most there is: the search's stack in
        # LDS then holds 63 entries behind a push, and its 64th slot carries the stack height to the other lanes
        levels = (want_peak + 2) // 3
        main = ref[25:30] + b"abcdefghijklmnopqrstuvwxyz"[:levels + 3]
        sib, pos = [], 6
        for level in range(levels):
            for c in b"XYZ"[:3 if level < levels - 1 else want_peak - 3 * (levels - 1)]:
                sib.append(rd(main[pos - k:pos] + bytes([c])))
            pos += 1

        def check(case, want_peak=want_peak, max_pending=max_pending):
            s, = case.want_asm()[0]["starts"]
            assert (s["peak"], s["status"], len(s["paths"])) == (want_peak, AR.GAVE_UP if want_peak > max_pending else AR.OK, 0), (s["peak"], s["status"])
        out.append(one("pending_%d" % want_peak, k, ref, sib + [rd(main)], check=check, ap=dict(k_last=0, max_pending=max_pending)))
    snp = [bubble(ref, 30, b"a", 1, k)]
    need = one("", k, ref, snp, ap=NO_RETRY).want_asm()[0]["starts"][0]["steps"]
    out.append(one("max_steps_at", k, ref, snp, check=expect(n_paths=1, n_steps=0), ap=dict(k_last=0, max_steps=need)))
    out.append(one("max_steps_below", k, ref, snp, check=expect(n_paths=0, n_steps=1), ap=dict(k_last=0, max_steps=need - 1)))
    k = 5
    for n in (WAVE - 1, WAVE, WAVE + 1, 1000):               # a path of n nodes: an insertion of n - k - 1 bases
        rng = np.random.default_rng(n)
        seen = set()
        ref5 = uniq(rng, 40, k, seen)
        ins = uniq(rng, n - k - 1, k, seen).lower()
        out.append(one("path_%d_nodes" % n, k, ref5, [bubble(ref5, 20, ins, 0, k)], check=expect(n_starts=1, n_paths=1, n_path_nodes=n), ap=NO_RETRY))
    for n in (0, WAVE + 1, 4 * WAVE + 1):                    # that many starts: a SNP every 14 bases
        long_ref = uniq(np.random.default_rng(100 + n), 14 * n + 30, k)
        reads = [bubble(long_ref, 14 * i + 15, b"a", 1, k) for i in range(n)]
        out.append(one("starts_%d" % n, k, long_ref, reads, check=expect(n_starts=n, n_paths=n), ap=NO_RETRY))
    by = {c.name: c for c in out}
    out.append(join("starts_of_several_windows", [by["starts_65"], by["starts_0"], by["path_64_nodes"], by["starts_257"], by["path_1000_nodes"]],
                    expect(n_starts=[65, 0, 1, 257, 1])))
    return out


def families():
    return {"cycles": cycle_cases(), "retry": retry_cases(), "paths": path_cases()}


def all_cases():
    out = [c for f in families().values() for c in f]
    assert len({c.name for c in out}) == len(out)
    return out


# ------------------------------------------------------------------------------------------------- the fixtures
def fixture(name):
    """(DbgReads, DbgWins) of tests/golden/<name>.bam / .fa over the whole contig ctg1"""
    from genomicsbench_amd import dbg as D
    rs, (ctg, beg, end), _ = D.read_bam(os.path.join(GOLDEN, name + ".bam"), "ctg1")
    seq = D.read_fasta(os.path.join(GOLDEN, name + ".fa"))[ctg]
    return rs, D.make_windows(rs, beg, end, seq)


_FIXTURES = {}


def fixture_want(name):
    """the restatement of every window of the fixture, computed once"""
    if name not in _FIXTURES:
        rs, ws = fixture(name)
        _FIXTURES[name] = [AR.window(ws.window_ref(w), int(ws.ref_pos[w]), [rs.read(r) for r in range(int(ws.read_lo[w]), int(ws.read_hi[w]))])
                           for w in range(ws.n_win)]
    return _FIXTURES[name]
