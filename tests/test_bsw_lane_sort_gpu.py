"""bsw lane path: the lane sort's lists, read back through gbx_debug_bsw_lane_lists, against a host restatement of the key
(lane_ok, lane_row, lane_key of bsw_kernels.hip), and the results against the oracle, all six fields.  The sorted order must
hold exactly the pairs the lane path takes, in non-decreasing key order, the key rows' first positions must be the host's
counts, and two runs must give the same order.  Sizes around the sort's tile T, one key across tiles and slabs, one row
across slabs, a pair in every row, the clamp of the seed score, the bounds of the formats and the classes, refused pairs,
a workspace used twice, both scorings, the sort in one and in two groups."""
import ctypes as C
import functools

import numpy as np
import pytest

from genomicsbench_amd import _native as N
from genomicsbench_amd.bsw import BswBatch, DeviceBswBatch, make_params
from oracle import oracle_py as O

pytestmark = pytest.mark.gpu

LANE_QMAX, SPLIT_Q = 159, 80
L_QROWS = LANE_QMAX + 1 - SPLIT_Q
L_ROWS = 2 * L_QROWS
LANE_ROWS = 2 * (LANE_QMAX + 1)
SCORINGS = {"default": {}, "asym": dict(o_del=5, e_del=2, o_ins=7, e_ins=3)}
MAX_TLEN = 65535                              # GBX_BSW_MAX_TLEN: a longer target is answered with -1 in every field
ARENA = 1 << 15


@pytest.fixture
def lane(monkeypatch):
    monkeypatch.setenv("GBX_BSW_LANE", "1")
    monkeypatch.setenv("GBX_BSW_DIRECT", "0")
    for name in ("GBX_BSW_SORT_SPLIT", "GBX_BSW_LANE_REG", "GBX_BSW_LANE_PRIO", "GBX_BSW_LANE_REG_WAVES"):
        monkeypatch.delenv(name, raising=False)


def tile():
    f = N.lib().gbx_debug_bsw_lane_sort_tile
    f.argtypes, f.restype = [], C.c_int
    return f()


@functools.lru_cache(maxsize=None)
def arenas():
    """Queries: random bases with a few N.  Targets: the same bases with 6 % substitutions, so that windows stay open."""
    rng = np.random.default_rng(77)
    q = rng.integers(0, 4, ARENA).astype(np.uint8)
    t = np.where(rng.random(ARENA) < 0.06, rng.integers(0, 4, ARENA), q).astype(np.uint8)
    q[rng.random(ARENA) < 0.002] = 4
    return t, q


def batch(qlen, h0, tlen=None, seed=0):
    """One pair per entry of qlen / h0 (broadcast against each other): query and target start at the same arena offset."""
    qlen, h0 = np.broadcast_arrays(np.asarray(qlen, dtype=np.int32), np.asarray(h0, dtype=np.int32))
    n = qlen.size
    rng = np.random.default_rng(seed)
    off = rng.integers(0, ARENA - 600, n).astype(np.int64)
    t, q = arenas()
    l1 = (qlen + rng.integers(0, 40, n)).astype(np.int32) if tlen is None else np.broadcast_to(np.asarray(tlen, dtype=np.int32), (n,)).copy()
    return BswBatch(t, q, off, off.copy(), l1, qlen.copy(), h0.copy())


def concat(*bs):
    cat = lambda f: np.concatenate([getattr(b, f) for b in bs])
    return BswBatch(bs[0].ref, bs[0].qer, cat("idr"), cat("idq"), cat("len1"), cat("len2"), cat("h0"))


def shuffled(b, seed):
    i = np.random.default_rng(seed).permutation(b.n)
    return BswBatch(b.ref, b.qer, b.idr[i], b.idq[i], b.len1[i], b.len2[i], b.h0[i])


def max_mat(scoring):
    """The largest entry of the scoring's matrix, as the device parameters hold it (never below 0 in the key)."""
    p = make_params(**SCORINGS[scoring])
    return max(0, max(int(p.mat[k]) for k in range(25)))


def host_keys(b, scoring="default"):
    """(taken, key) per pair: lane_ok, the sort's bound on the target and lane_key restated."""
    q, h = b.len2.astype(np.int64), b.h0.astype(np.int64)
    bound = h + q * max_mat(scoring)
    taken = (q >= 1) & (q <= LANE_QMAX) & (b.len1 >= 1) & (b.len1 <= MAX_TLEN) & (h >= 0) & (bound < 8192)
    wide = (bound >= 256).astype(np.int64)
    row = np.where(q >= SPLIT_Q, wide * L_QROWS + q - SPLIT_Q, L_ROWS + wide * SPLIT_Q + q)
    return taken, (row << 8) | np.minimum(h, 255)


def lists(d):
    order = np.full(d.n, -1, dtype=np.int32)
    first = np.full(LANE_ROWS + 1, -1, dtype=np.int32)
    f = N.lib().gbx_debug_bsw_lane_lists
    f.argtypes, f.restype = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p], C.c_int
    N.check(f(d.work.data_ptr(), d.n, N.ptr(order), N.ptr(first)))
    return order, first


def check_lists(b, order, first, what, scoring="default"):
    taken, key = host_keys(b, scoring)
    counts = np.bincount(key[taken] >> 8, minlength=LANE_ROWS)
    want_first = np.concatenate([[0], np.cumsum(counts)])
    assert np.array_equal(first, want_first), "%s: key rows' first positions; first difference at row %d" % (
        what, int(np.nonzero(first != want_first)[0][0]))
    total = int(first[LANE_ROWS])
    got = order[:total].astype(np.int64)
    assert np.array_equal(np.sort(got), np.nonzero(taken)[0]), "%s: the order is not a permutation of the lane path's pairs" % what
    assert np.all(np.diff(key[got]) >= 0), "%s: keys decrease along the order" % what


def run(p, d):
    import torch
    d.out.fill_(-7)
    d.run(p, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d.results()


def check(monkeypatch, b, scoring="default", splits=("0", "1"), d=None):
    """b with the sort in one group and in two: lists, the same order on a second run, results against the oracle."""
    import torch
    p = make_params(**SCORINGS[scoring])
    ok = np.nonzero(b.len1 <= MAX_TLEN)[0]
    sub = b if ok.size == b.n else BswBatch(b.ref, b.qer, b.idr[ok], b.idq[ok], b.len1[ok], b.len2[ok], b.h0[ok])
    oracle = O.bsw_oracle(p, sub, 8)
    want = np.full((b.n,) + oracle.shape[1:], -1, dtype=oracle.dtype)
    want[ok] = oracle
    d = d or DeviceBswBatch(b, torch.device("cuda:0"))
    for split in splits:
        monkeypatch.setenv("GBX_BSW_SORT_SPLIT", split)
        got = run(p, d)
        order, first = lists(d)
        what = "n=%d split=%s" % (b.n, split)
        check_lists(b, order, first, what, scoring)
        assert np.array_equal(got, want), "%s: %d pairs differ from the oracle" % (what, int((got != want).any(1).sum()))
        again = run(p, d)
        order2, first2 = lists(d)
        total = int(first[LANE_ROWS])
        assert np.array_equal(order[:total], order2[:total]) and np.array_equal(first, first2), "%s: the second run's order differs" % what
        assert np.array_equal(again, want)
    return d


def mixed(n, seed):
    """n pairs over all query lengths and both formats, seed scores on both sides of the clamp."""
    rng = np.random.default_rng(seed)
    q = rng.integers(1, LANE_QMAX + 1, n)
    h = np.where(rng.random(n) < 0.3, rng.integers(200, 320, n), rng.integers(0, 120, n))
    return batch(q, h, seed=seed)


@pytest.mark.parametrize("where", ["1", "63", "64", "65", "T-1", "T", "T+1", "2T+17"])
def test_sizes_around_a_wavefront_and_a_tile(lane, monkeypatch, where):
    T = tile()
    n = {"T-1": T - 1, "T": T, "T+1": T + 1, "2T+17": 2 * T + 17}.get(where) or int(where)
    check(monkeypatch, mixed(n, 100 + n % 97))


def test_one_key_across_tiles_and_slabs(lane, monkeypatch):
    """3T + 5 pairs of one key: one bin of one row, in every tile of level 1 and every slab of level 2."""
    check(monkeypatch, batch(np.full(3 * tile() + 5, 60), 30, seed=1))


@pytest.mark.parametrize("fmt", ["compact", "wide"])
def test_one_row_across_slabs(lane, monkeypatch, fmt):
    """2T pairs of one row, seed scores over the row's whole range: a compact row (h0 + qlen < 256) has its widest range, 0..254,
    at a query of one base; a wide row of 159 bases holds 97 and up, and everything from 255 on in its last bin."""
    n = 2 * tile()
    rng = np.random.default_rng(2)
    b = batch(1, rng.integers(0, 255, n), seed=2) if fmt == "compact" else batch(LANE_QMAX, rng.integers(97, 400, n), seed=3)
    taken, key = host_keys(b)
    assert taken.all() and len(set(key >> 8)) == 1 and len(set(key & 255)) > 150
    check(monkeypatch, b)


@pytest.mark.parametrize("scoring", sorted(SCORINGS))
def test_a_pair_in_every_row(lane, monkeypatch, scoring):
    """Queries of 1..159 bases with seed scores 40 (compact) and 240 (wide from 16 bases on)."""
    q = np.arange(1, LANE_QMAX + 1)
    b = shuffled(concat(batch(q, 40, seed=4), batch(q, 240, seed=5)), 6)
    taken, key = host_keys(b, scoring)
    assert taken.all() and len(set(key >> 8)) == 2 * LANE_QMAX - 15
    check(monkeypatch, b, scoring)


def test_the_clamp_of_the_seed_score(lane, monkeypatch):
    """Seed scores 0, 254, 255, 256 and 300 at one query length: 255 and up share the row's last bin."""
    b = shuffled(batch(20, np.repeat([0, 254, 255, 256, 300], 40), seed=7), 8)
    assert len(set(host_keys(b)[1])) == 3
    check(monkeypatch, b)


def test_the_bound_between_the_formats(lane, monkeypatch):
    """h0 + qlen = 255 (compact) and 256 (wide), at queries on both sides of the group cut."""
    q = np.repeat([30, 30, 90, 90], 50)
    b = shuffled(batch(q, np.repeat([225, 226, 165, 166], 50), seed=9), 10)
    assert len(set(host_keys(b)[1] >> 8)) == 4
    check(monkeypatch, b)


@pytest.mark.parametrize("scoring", sorted(SCORINGS))
def test_class_bounds_and_the_longest_query(lane, monkeypatch, scoring):
    """Queries of 79 / 80, 99 / 100, 135 / 136 and 159 / 160 bases in both formats; 160 bases go to the row kernels."""
    q = np.repeat([79, 80, 99, 100, 135, 136, 159, 160], 42)
    b = shuffled(batch(q, np.where(np.arange(q.size) % 2 == 0, 40, 240), seed=11), 12)
    taken, _ = host_keys(b, scoring)
    assert int((~taken).sum()) == 42
    check(monkeypatch, b, scoring)


@pytest.mark.parametrize("scoring", sorted(SCORINGS))
def test_refused_pairs_are_absent_and_answered(lane, monkeypatch, scoring):
    """Negative seed scores, empty targets, h0 + qlen of 8192 and more and queries beyond 159 among pairs the lane path takes."""
    ok = mixed(1500, 13)
    q = np.random.default_rng(14).integers(1, LANE_QMAX + 1, 400)
    neg = batch(q[:100], -1 - np.arange(100) % 5, seed=15)
    empty = batch(q[100:200], 50, tlen=0, seed=16)
    big = batch(q[200:300], 8192 - q[200:300] + np.arange(100) % 3, seed=17)
    long_q = batch(160 + np.arange(100) % 90, 40, seed=18)
    b = shuffled(concat(ok, neg, empty, big, long_q), 19)
    assert int(host_keys(b, scoring)[0].sum()) == ok.n
    check(monkeypatch, b, scoring)


def test_targets_at_and_beyond_the_longest(lane, monkeypatch):
    """Targets of GBX_BSW_MAX_TLEN bases are sorted and extended; one base more and the pair is in no list and answered with -1."""
    rng = np.random.default_rng(23)
    size = 1 << 17
    q = rng.integers(0, 4, size).astype(np.uint8)
    t = np.where(rng.random(size) < 0.06, rng.integers(0, 4, size), q).astype(np.uint8)
    n = 300
    qlen = rng.integers(1, LANE_QMAX + 1, n).astype(np.int32)
    tlen = (qlen + rng.integers(0, 40, n)).astype(np.int32)
    tlen[0:60:3], tlen[1:60:3] = MAX_TLEN, MAX_TLEN + 1
    off = rng.integers(0, size - MAX_TLEN - 1, n).astype(np.int64)
    b = BswBatch(t, q, off, off.copy(), tlen, qlen, rng.integers(0, 300, n).astype(np.int32))
    taken, _ = host_keys(b)
    assert int((~taken).sum()) == 20 and int((b.len1 == MAX_TLEN).sum()) == 20
    check(monkeypatch, b)


@pytest.mark.parametrize("split", ["0", "1"])
def test_one_workspace_twice(lane, monkeypatch, split):
    """Two jobs of as many pairs with other row populations on one workspace, then the first again: nothing is left over."""
    import torch
    n = tile() + 300
    a = batch(np.random.default_rng(20).integers(100, 160, n), 20, seed=20)
    b = batch(np.random.default_rng(21).integers(1, 60, n), np.random.default_rng(22).integers(0, 300, n), seed=21)
    dev = torch.device("cuda:0")
    da, db = DeviceBswBatch(a, dev), DeviceBswBatch(b, dev)
    db.work, db.work_bytes = da.work, da.work_bytes
    for bt, d in ((a, da), (b, db), (a, da)):
        check(monkeypatch, bt, splits=(split,), d=d)
