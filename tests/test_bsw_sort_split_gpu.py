"""bsw lane path: the lane sort in two groups by query length (GBX_BSW_SORT_SPLIT=1 - group L: queries 80..159 of both formats,
sorted first, its launches behind an event of their own; group S: the rest) against the single sort (the default, and
GBX_BSW_SORT_SPLIT=0) and the oracle, all six fields.  Both sorts share the key layout (group L's rows first): where the groups
and the classes meet, a group that is empty, group totals around a wavefront's 64 pairs, pairs the lane path refuses, and a
workspace that is used twice."""
import functools

import numpy as np
import pytest

from genomicsbench_amd import _native as N
from genomicsbench_amd.bsw import BswBatch, DeviceBswBatch, make_params
from genomicsbench_amd.datagen import gen_bsw
from oracle import oracle_py as O
from cases import adversarial_bsw

pytestmark = pytest.mark.gpu

SPLIT_Q = 80                   # LANE_SPLIT_Q in bsw_kernels.hip: group L = queries from here on
LANE_QMAX = 159
# the last query length of a class and the first of the next, both formats; 159 / 160 = lane kernels / row kernels
STRADDLE = (39, 40, 47, 48, 79, 80, 99, 100, 103, 104, 127, 128, 135, 136, 159, 160)

SCORINGS = {"default": {}, "asym": dict(o_del=5, e_del=2, o_ins=7, e_ins=3)}      # bwa's defaults; the kernels' non-SYM instances


@pytest.fixture
def lane(monkeypatch):
    monkeypatch.setenv("GBX_BSW_LANE", "1")
    monkeypatch.setenv("GBX_BSW_DIRECT", "0")
    for name in ("GBX_BSW_SORT_SPLIT", "GBX_BSW_LANE_REG", "GBX_BSW_LANE_PRIO", "GBX_BSW_LANE_REG_WAVES"):      # the defaults
        monkeypatch.delenv(name, raising=False)


@functools.lru_cache(maxsize=None)
def reads():
    """Generated 151-bp extensions: queries of 1..130, seed scores that keep every pair in the compact format."""
    return gen_bsw(8000, 4242)


@functools.lru_cache(maxsize=None)
def long_queries():
    """Adversarial pairs whose queries have at least 160 bases: a prefix gives any query length of the lane path."""
    b = adversarial_bsw(500, 97, max_q=250, max_t=400)
    return take(b, np.nonzero(b.len2 >= LANE_QMAX + 1)[0])


def take(b, idx, len2=None, h0=None):
    """The pairs `idx` of b, with query lengths (a prefix of the query) and seed scores replaced where given."""
    idx = np.asarray(idx, dtype=np.int64)
    l2 = b.len2[idx] if len2 is None else np.minimum(b.len2[idx], np.asarray(len2, dtype=np.int32))
    return BswBatch(b.ref, b.qer, b.idr[idx], b.idq[idx], b.len1[idx], l2, b.h0[idx] if h0 is None else np.asarray(h0, dtype=np.int32))


def concat(*bs):
    ro = np.cumsum([0] + [b.ref.size for b in bs[:-1]])
    qo = np.cumsum([0] + [b.qer.size for b in bs[:-1]])
    cat = lambda f: np.concatenate([getattr(b, f) for b in bs])
    return BswBatch(cat("ref"), cat("qer"), np.concatenate([b.idr + o for b, o in zip(bs, ro)]),
                    np.concatenate([b.idq + o for b, o in zip(bs, qo)]), cat("len1"), cat("len2"), cat("h0"))


def shuffled(b, seed):
    return take(b, np.random.default_rng(seed).permutation(b.n))


def group_sizes(b, max_mat=1):
    """Pairs the lane path takes, by (group, format): {("L", "c"): n, ...} - the library's rule (lane_ok, lane_key)."""
    bound = b.h0.astype(np.int64) + b.len2.astype(np.int64) * max_mat
    ok = (b.len2 >= 1) & (b.len2 <= LANE_QMAX) & (b.len1 >= 1) & (b.h0 >= 0) & (bound < 8192)
    out = {}
    for g, gm in (("L", b.len2 >= SPLIT_Q), ("S", b.len2 < SPLIT_Q)):
        for f, fm in (("c", bound < 256), ("w", bound >= 256)):
            out[g, f] = int((ok & gm & fm).sum())
    return out


def run_device(p, d):
    """One launch of a resident batch -> (results, launches of the stage bsw_lane_sort: one per sorted group)."""
    import torch
    N.profile_begin()
    d.run(p, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    prof = N.profile_end(256)
    return d.results(), prof.get("bsw_lane_sort", (0.0, 0))[1]


def assert_same(got, want, b, what):
    if not np.array_equal(got, want):
        rows = np.nonzero((got != want).any(1))[0]
        k = int(rows[0])
        raise AssertionError("%s: %d/%d pairs differ; first k=%d got=%s want=%s (len1=%d len2=%d h0=%d)"
                             % (what, len(rows), len(want), k, got[k], want[k], b.len1[k], b.len2[k], b.h0[k]))


def check(monkeypatch, p, b):
    """b with the sort in two groups and in one, against the oracle and each other."""
    import torch
    assert 1 <= b.n <= 4000
    want = O.bsw_oracle(p, b, 8)
    d = DeviceBswBatch(b, torch.device("cuda:0"))
    monkeypatch.setenv("GBX_BSW_SORT_SPLIT", "1")
    on, sorts_on = run_device(p, d)
    monkeypatch.setenv("GBX_BSW_SORT_SPLIT", "0")
    off, sorts_off = run_device(p, d)
    monkeypatch.delenv("GBX_BSW_SORT_SPLIT", raising=False)
    default, sorts_default = run_device(p, d)
    assert on.shape == (b.n, len(N.BSW_RESULT_FIELDS))
    assert (sorts_on, sorts_off, sorts_default) == (2, 1, 1), \
        "sorted groups: %d with GBX_BSW_SORT_SPLIT=1, %d with 0, %d by default" % (sorts_on, sorts_off, sorts_default)
    assert_same(on, want, b, "two groups vs oracle")
    assert_same(off, want, b, "one sort vs oracle")
    assert_same(default, want, b, "the default vs oracle")


def both_formats(b, every=3, h0=230):
    """Every `every`-th pair's seed score raised so that it is a wide pair (h0 + qlen >= 256 from 26 bases on)."""
    h = b.h0.copy()
    h[::every] = h0
    return take(b, np.arange(b.n), h0=h)


@pytest.mark.parametrize("scoring", sorted(SCORINGS))
@pytest.mark.parametrize("group", ["L", "S"])
def test_every_pair_in_one_group(lane, monkeypatch, scoring, group):
    """The other group's sort counts, scans and places nothing, and its launches find empty lists; both formats."""
    r = reads()
    m = r.len2 >= SPLIT_Q if group == "L" else (r.len2 >= 26) & (r.len2 < SPLIT_Q)
    b = both_formats(take(r, np.nonzero(m)[0][:1500]))
    sizes = group_sizes(b)
    other = "S" if group == "L" else "L"
    assert sizes[group, "c"] > 128 and sizes[group, "w"] > 128 and sizes[other, "c"] == sizes[other, "w"] == 0, sizes
    check(monkeypatch, make_params(**SCORINGS[scoring]), b)


@pytest.mark.parametrize("scoring", sorted(SCORINGS))
@pytest.mark.parametrize("empty", [("L", "w"), ("S", "w"), ("L", "c"), ("S", "c")])
def test_one_group_empty_in_one_format(lane, monkeypatch, scoring, empty):
    """Both groups hold pairs, one of them in one format only: the empty stretch lies between two that are not."""
    r = reads()
    r = take(r, np.nonzero(r.len2 >= 26)[0][:2400])
    in_group = r.len2 >= SPLIT_Q if empty[0] == "L" else r.len2 < SPLIT_Q
    h = both_formats(r).h0
    if empty[1] == "w":
        h = np.where(in_group, r.h0, h)                 # the group's pairs stay compact
    else:
        h = np.where(in_group, 230, h)                  # the group's pairs are all wide
    b = take(r, np.arange(r.n), h0=h)
    sizes = group_sizes(b)
    assert sizes[empty] == 0 and all(v > 64 for k, v in sizes.items() if k != empty), sizes
    check(monkeypatch, make_params(**SCORINGS[scoring]), b)


@pytest.mark.parametrize("scoring", sorted(SCORINGS))
def test_query_lengths_at_the_cut_and_every_class_bound(lane, monkeypatch, scoring):
    """Queries of 39/40 .. 159/160 bases, each length in the compact and in the wide format (seed score 40 and 240: the same
    query length on either side of 256 in both groups), 21 pairs a length and format; 160 bases go to the row kernels."""
    lq = long_queries()
    assert lq.n >= 42, lq.n
    parts = []
    for k, ql in enumerate(STRADDLE):
        idx = (np.arange(42) * 7 + k * 5) % lq.n
        parts.append(take(lq, idx, len2=np.full(42, ql), h0=np.where(np.arange(42) % 2 == 0, 40, 240)))
    b = shuffled(concat(*parts), 5)
    assert set(STRADDLE) == set(int(v) for v in b.len2)
    sizes = group_sizes(b)
    assert sizes == {("L", "c"): 210, ("L", "w"): 210, ("S", "c"): 105, ("S", "w"): 105}, sizes
    check(monkeypatch, make_params(**SCORINGS[scoring]), b)


@pytest.mark.parametrize("totals", [(64, 65), (65, 1), (1, 64), (100, 37), (0, 1), (1, 0)])
def test_group_totals_around_a_wavefront(lane, monkeypatch, totals):
    """Group totals of exactly 64, 65 and 1 pairs and ragged ones, (L, S): one class each, so the total is a launch's list."""
    r = reads()
    nl, ns = totals
    il = np.nonzero((r.len2 >= 100) & (r.len2 <= 127))[0][:nl]
    is_ = np.nonzero((r.len2 >= 48) & (r.len2 <= 79))[0][:ns]
    b = shuffled(take(r, np.concatenate([il, is_])), 11)
    sizes = group_sizes(b)
    assert (sizes["L", "c"], sizes["S", "c"], sizes["L", "w"], sizes["S", "w"]) == (nl, ns, 0, 0), sizes
    check(monkeypatch, make_params(), b)


@pytest.mark.parametrize("scoring", sorted(SCORINGS))
def test_refused_pairs_among_the_groups(lane, monkeypatch, scoring):
    """Pairs the lane path turns down (negative seed score, empty target, score bound of 8192 and more, queries beyond 159)
    between pairs of both groups and formats: row kernels and lane kernels write one output array."""
    r = reads()
    lanes = both_formats(take(r, np.nonzero(r.len2 >= 26)[0][:1901]))
    ref = take(r, np.arange(3000, 3240))
    h = ref.h0.copy()
    l1 = ref.len1.copy()
    h[0::3] = -1 - (np.arange(len(h[0::3])) % 5)
    l1[1::3] = 0
    h[2::3] = 8192 - ref.len2[2::3] + (np.arange(len(h[2::3])) % 3)         # h0 + qlen = 8192, 8193, 8194
    refused = BswBatch(ref.ref, ref.qer, ref.idr, ref.idq, l1, ref.len2, h)
    b = shuffled(concat(lanes, refused, long_queries()), 23)
    sizes = group_sizes(b)
    assert all(v > 64 for v in sizes.values()) and sum(sizes.values()) == lanes.n, sizes
    assert any(v % 64 for v in (sizes["L", "c"] + sizes["L", "w"], sizes["S", "c"] + sizes["S", "w"]))
    check(monkeypatch, make_params(**SCORINGS[scoring]), b)


@pytest.mark.parametrize("split", ["1", "0"])
def test_one_workspace_twice_with_other_group_sizes(lane, monkeypatch, split):
    """Two launches of as many pairs on one workspace: most pairs in group L, then most in group S, then the first again.
    Counts, list bases or chunk cursors left from the call before would move or shorten a list."""
    import torch
    monkeypatch.setenv("GBX_BSW_SORT_SPLIT", split)
    p = make_params()
    r = reads()
    il, is_ = np.nonzero(r.len2 >= SPLIT_Q)[0], np.nonzero((r.len2 >= 26) & (r.len2 < SPLIT_Q))[0]
    a = both_formats(shuffled(take(r, np.concatenate([il[:1400], is_[:100]])), 3))
    b = both_formats(shuffled(take(r, np.concatenate([il[1400:1530], is_[100:1470]])), 4), every=2)
    assert a.n == b.n and group_sizes(a) != group_sizes(b)
    dev = torch.device("cuda:0")
    d, other = DeviceBswBatch(a, dev), DeviceBswBatch(b, dev)
    work = d.work
    for k, (batch, src) in enumerate(((a, d), (b, other), (a, d))):
        src.work, src.work_bytes = work, d.work_bytes
        src.out.fill_(-7)
        got, sorts = run_device(p, src)
        assert sorts == (2 if split == "1" else 1)
        assert_same(got, O.bsw_oracle(p, batch, 8), batch, "call %d on the shared workspace" % k)
