"""The calls of tests/chain_cases.py are what they claim to be, shown on the CPU alone: the restatement tests/chain_ref.py
equals the oracle (and the compiled reference where it exists) on every case, every case's claim about the kernel paths it
reaches holds on the restatement's fact list, every mutant of the restatement is caught by a named case, and the restated
cut rule gives jobs that are independent calls.  tests/test_chain_edges_gpu.py runs the same calls on the device."""
import numpy as np
import pytest

import chain_cases as CC
import chain_ref as CR
from cases import chain_pack
from oracle import oracle_py as O

FAMILIES = list(CC.families())
NAMES = ("score", "parent", "target", "peak")


def same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert np.array_equal(g, w), "%s: %s differs first at anchor %d" % (what, name, int(np.argmax(g != w)))


@pytest.mark.parametrize("family", FAMILIES)
def test_restatement_equals_the_oracle(family):
    """all five outputs, case by case and as the packed call list the device test runs"""
    cases = CC.families()[family]
    pairs = 0
    for c in cases:
        want = O.chain_oracle(*chain_pack([c.call]), return_pairs=True)
        got = c.ref(c.rings[0])
        same(got[:4], want[:4], c.name)
        assert got[4] == want[4], (c.name, got[4], want[4])
        pairs += got[4]
    packed = O.chain_oracle(*CC.pack(cases), return_pairs=True)
    same([np.concatenate([c.ref(c.rings[0])[k] for c in cases]) for k in range(4)], packed[:4], family)
    assert packed[4] == pairs


@pytest.mark.skipif(O.ref_lib("chain") is None, reason="compiled reference only exists in the build container")
@pytest.mark.parametrize("family", FAMILIES)
def test_restatement_equals_the_live_reference(family):
    for c in CC.families()[family]:
        same(c.ref(c.rings[0])[:4], O.chain_ref(*chain_pack([c.call])), c.name)


@pytest.mark.parametrize("family", FAMILIES)
def test_claims(family):
    """every case reaches the kernel path it is named for, at the ring sizes it is meant for; the outputs do not depend
    on the ring"""
    for c in CC.families()[family]:
        for ring in c.rings:
            res = c.ref(ring)
            c.claim(c, ring, res)
            same(res[:4], c.ref(c.rings[0])[:4], c.name)


def test_every_tier_shape_and_break_position_occurs():
    """the cross table the families are built for, read from the fact lists"""
    seen = set()
    for fam in ("lookback", "breaks", "shapes", "marks"):
        for c in CC.families()[fam]:
            for ring in c.rings:
                for r in c.ref(ring)[5]:
                    seen.add(("tier", r["tier"], ring))
                    if r["nopen"]:
                        seen.add(("shape", r["shape"], "window" if r["c"] == 0 else "later"))
                    if r["brk"] is not None:
                        seen.add(("break", r["tier"], ring))
                        seen.add(("break lane", r["brk"] if r["brk"] in (0, 63) else "mid"))
                    for m in r["marks"]:
                        seen.add(("mark", m[2], ring))
                        if m[1] in (r["live0"], r["live0"] - 1):
                            seen.add(("mark at", m[1] - r["live0"], ring))
                    for h in r["hits"]:
                        seen.add(("hit", h[1], r["tier"], ring))
    want = {("shape", s, w) for s in ("quiet", "popcount", "lead", "scan") for w in ("window", "later")}
    want |= {("break lane", b) for b in (0, 63, "mid")}
    for ring in CR.RINGS:
        want |= {("tier", t, ring) for t in ("window", "ring", "straddle", "global", "ring_tail")}
        want |= {("break", t, ring) for t in ("window", "ring", "straddle", "global")}
        want |= {("mark", "ring", ring), ("mark", "direct", ring), ("mark at", 0, ring), ("mark at", -1, ring)}
        want |= {("hit", "same", "window", ring), ("hit", "ring", "ring", ring), ("hit", "ring", "straddle", ring),
                 ("hit", "global", "straddle", ring), ("hit", "global", "global", ring), ("hit", "same", "global", ring)}
    assert not want - seen, sorted(map(str, want - seen))


# mutant of the restatement -> cases that must tell it from the restatement (each at the first ring it is meant for)
CATCHES = {
    "no_round": ("unsorted_two", "unsorted_300"),
    "mark_behind_break": ("break_window_mid_bait", "break_ring_mid", "break_straddle_mid_bait_r512", "break_global_mid_bait_r768"),
    "improve_behind_break": ("break_window_mid_bait", "break_ring_l0_bait", "break_straddle_mid_bait_r512", "break_global_mid_bait_r768",
                             "marks_straddle_r768"),
    "nskip_unclamped": ("break_window_l63", "break_global_l63_r512"),
    "no_global_hits": ("marks_straddle_r512", "marks_global_r768"),
    "no_direct_stores": ("marks_straddle_r512", "marks_global_scan_r768", "break_straddle_l63_r768"),
    "window_ignores_own_marks": ("break_window_mid_bait", "break_window_l63", "shape_scan_window_reflect"),
    "clin_fp32": ("gap_aq100", "gap_aq12.5"),
    "dq_limit": ("fold_dq_lim_x", "fold_dq_lim_y"),
    "dr_limit": ("fold_dr_lim_segs2",),
    "bw_limit": ("fold_bw0", "fold_bw30"),
    "max_iter": ("max_iter",),
}


@pytest.mark.parametrize("mutant", CR.MUTANTS)
def test_every_mutant_is_caught_by_a_named_case(mutant):
    by_name = {c.name: c for cases in CC.families().values() for c in cases}
    assert CATCHES[mutant]
    for name in CATCHES[mutant]:
        c = by_name[name]
        good = c.ref(c.rings[0])
        bad = CR.chain_dp(*c.call, ring=c.rings[0], mutant=mutant, want_facts=False)
        assert any(not np.array_equal(g, b) for g, b in zip(good[:4], bad[:4])) or good[4] != bad[4], (mutant, name)


def test_the_two_anchor_unsorted_call():
    c = CC.unsorted_two()
    s, p, t, k, pairs = O.chain_oracle(*chain_pack([c.call]), return_pairs=True)
    assert (list(s), list(p), list(t), list(k), pairs) == ([15, 41], [-1, 0], [0, 0], [15, 41], 1)
    assert list(CR.chain_dp(*c.call, mutant="no_round")[0]) == [15, 42]


@pytest.mark.parametrize("family", ["cuts", "unsorted", "lookback", "folds"])
def test_jobs_of_the_restated_cut_rule_are_calls_of_their_own(family):
    """cutting a call into its jobs, running each job as a call and adding the job's start to parents and targets gives
    the uncut result; unmarked targets stay 0"""
    n_cut = 0
    for c in CC.families()[family]:
        whole = c.ref(c.rings[0])
        jobs = whole[6]
        assert jobs[0][0] == 0 and sum(n for _, n, _ in jobs) == len(c.x)
        one_key = len({(int(x) >> 32, int(y) >> 48 & 0xff) for x, y in zip(c.x, c.y)}) == 1
        is_sorted = bool(np.all(c.x[:-1] <= c.x[1:]))
        assert CR.chain_jobs(*c.call, split=False) == [(0, len(c.x), one_key and is_sorted)]
        assert is_sorted or len(jobs) == 1
        assert not any(nar for _, _, nar in CR.chain_jobs(*c.call, wide=True))
        n_cut += len(jobs) > 1
        pairs = 0
        for s, n, _ in jobs:
            s_, p_, t_, k_, ev = O.chain_oracle(*chain_pack([(c.x[s:s + n], c.y[s:s + n], c.hdr)]), return_pairs=True)
            pairs += ev
            p_ = np.where(p_ >= 0, p_ + s, p_)
            marked = np.zeros(n, dtype=bool)
            marked[p_[p_ >= 0] - s] = True                   # only a parent can be marked
            assert not t_[~marked].any()
            t_ = np.where(t_ > 0, t_ + s, 0) if s else t_
            same((s_, p_, t_, k_), [a[s:s + n] for a in whole[:4]], "%s job at %d" % (c.name, s))
        assert pairs == whole[4], c.name
    assert n_cut
