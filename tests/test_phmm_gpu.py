"""GPU parity tests for phmm: HIP kernels (through the C-ABI) vs the oracle, 1e-5 relative on log10 likelihoods."""
import numpy as np
import pytest

from genomicsbench_amd.datagen import gen_phmm
from genomicsbench_amd.phmm import DevicePhmmBatchSet, PhmmBatchSet, forward_host
from oracle import oracle_py as O

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=["0", "1"])
def job_mode(request, monkeypatch):
    """Jobs under 12 000 pairs take the one-pair-per-wavefront kernels (GBX_PHMM_SMALL=1) instead of the grouped
    stream kernels (0); the cases here are small, so every test runs both ways."""
    monkeypatch.setenv("GBX_PHMM_SMALL", request.param)
    return request.param
# BASELINE.json north_star: "within 1e-5 relative for phmm float".  The reference computes
# log10f(result) - log10f(2^120) in float32, where log10f(result) ~ 36: one float ulp there is 3.8e-6
# ABSOLUTE, so two correct implementations (GKL's own AVX and scalar builds included) can differ by that
# much on a log-likelihood of any magnitude.  The bound is therefore 1e-5 relative with |want| floored at 1.
RTOL = 1e-5


def assert_close(got, want):
    fin = np.isfinite(want)
    # a read far longer than the haplotype underflows even the fp64 pass: both sides must say -inf
    assert np.array_equal(np.isfinite(got), fin) and np.array_equal(got[~fin], want[~fin]), "non-finite pattern differs"
    got, want = got[fin], want[fin]
    err = np.abs(got - want) / np.maximum(np.abs(want), 1.0)
    k = int(np.argmax(err))
    assert err[k] <= RTOL, "max rel err %.3g at pair %d: got %.9g want %.9g" % (err[k], k, got[k], want[k])


def make_set(reads, haps, quals=None, seed=0):
    """One batch from python strings; every read against every haplotype."""
    rng = np.random.default_rng(seed)
    cat = lambda xs: np.concatenate([np.frombuffer(x.encode(), dtype=np.uint8) for x in xs] + [np.zeros(8, np.uint8)])
    rl = [len(r) for r in reads]
    hl = [len(h) for h in haps]
    n = sum(rl)
    q = rng.integers(6, 42, n + 8).astype(np.uint8) if quals is None else np.full(n + 8, quals, np.uint8)
    qi = rng.integers(30, 50, n + 8).astype(np.uint8)
    qd = rng.integers(30, 50, n + 8).astype(np.uint8)
    qc = np.full(n + 8, 10, np.uint8)
    roff = np.concatenate([[0], np.cumsum(rl)])[:-1]
    hoff = np.concatenate([[0], np.cumsum(hl)])[:-1]
    return PhmmBatchSet([len(reads)], [len(haps)], roff, rl, cat(reads), q, qi, qd, qc, hoff, hl, cat(haps))


def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(list(alphabet), n))


def test_generated_batches():
    bs = gen_phmm(40, 3001)
    want, nd = O.phmm_oracle(bs, 8, True)
    assert_close(forward_host(bs), want)


def test_row_classes_and_tiles():
    """Read lengths across every rows-per-lane class, incl. reads longer than one 512-row tile."""
    rng = np.random.default_rng(1)
    reads, haps = [], [rand_seq(rng, 37), rand_seq(rng, 200, "ACGTN"), rand_seq(rng, 451), rand_seq(rng, 1300)]
    for R in (1, 2, 3, 63, 64, 65, 127, 128, 129, 151, 191, 192, 193, 255, 256, 257, 383, 384, 385, 511, 512, 513, 700, 1100):
        src = haps[3][7: 7 + R]
        reads.append("".join(c if rng.random() > 0.03 else "ACGT"[int(rng.integers(4))] for c in src))
    bs = make_set(reads, haps, seed=2)
    assert_close(forward_host(bs), O.phmm_oracle(bs, 8))


def test_stream_units_segments_and_lane_classes():
    """The stream path: read lengths on both sides of every 31-rows-per-lane class edge (and past its 248-row
    limit), 37 haplotypes per read - at this job's size phmm_launch puts one pair in a unit, so each of them is a
    unit of its own -, an odd number of units (idle half wavefront), very short haplotypes between long ones, and
    pairs in scrambled order.  Units of several pairs: test_phmm_units_gpu.py."""
    rng = np.random.default_rng(11)
    base = rand_seq(rng, 700)
    haps = []
    for k in range(37):
        H = int(rng.integers(1, 12)) if k % 5 == 0 else int(rng.integers(40, 460))
        o = int(rng.integers(0, 200))
        haps.append("".join(c if rng.random() > 0.02 else "ACGTN"[int(rng.integers(5))] for c in base[o:o + H]))
    reads = []
    for R in (1, 30, 31, 32, 61, 62, 63, 93, 94, 124, 125, 151, 155, 156, 186, 187, 217, 218, 247, 248, 249, 256, 300):
        o = int(rng.integers(0, 300))
        reads.append("".join(c if rng.random() > 0.03 else "ACGT"[int(rng.integers(4))] for c in base[o:o + R]))
    bs = make_set(reads, haps, seed=12)
    want = O.phmm_oracle(bs, 8)
    assert_close(forward_host(bs), want)
    # the same pairs in a scrambled order, a third of them dropped
    perm = rng.permutation(bs.n_pairs)[: 2 * bs.n_pairs // 3]
    sub = PhmmBatchSet.__new__(PhmmBatchSet)
    sub.__dict__.update(bs.__dict__)
    sub.pair_read, sub.pair_hap = bs.pair_read[perm].copy(), bs.pair_hap[perm].copy()
    sub.n_pairs = len(perm)
    sub.batch_pair_off = np.array([0, len(perm)], dtype=np.int64)
    assert_close(forward_host(sub), want[perm])


def test_fp64_fallback_pairs():
    rng = np.random.default_rng(3)
    haps = [rand_seq(rng, 120), rand_seq(rng, 300)]
    reads = [rand_seq(rng, 100), rand_seq(rng, 151), "A" * 70, rand_seq(rng, 300), haps[0][:90]]
    bs = make_set(reads, haps, quals=40, seed=4)
    want, nd = O.phmm_oracle(bs, 4, True)
    assert nd >= 4, "expected unrelated read/haplotype pairs to need the fp64 redo"
    assert_close(forward_host(bs), want)


def test_n_bases_and_single_cells():
    bs = make_set(["A", "N", "C", "ACGTN"], ["A", "N", "T", "NNNNN", "ACGTA"], seed=5)
    assert_close(forward_host(bs), O.phmm_oracle(bs))


def test_bytes_outside_acgtn_compare_literally():
    """The scalar semantics compare literal bytes (PairHMMUnitTest.cpp / oracle: `rs == hap || rs == 'N' || hap == 'N'`).  The
    stream kernels' prior tables know A C G T N only: a haplotype with any other byte is sent to the fp64 pass, which compares
    bytes; a READ with other bytes needs nothing special (it matches no coded symbol but N)."""
    rng = np.random.default_rng(11)
    core = rand_seq(rng, 90)
    haps = [core, core[:40].lower() + core[40:], core[:30] + "R" + core[31:], core.replace("A", "a"), rand_seq(rng, 70, "ACGTN")]
    reads = [core[5:80], core[5:80].lower(), core[10:60].replace("C", "c"), core[20:85], rand_seq(rng, 60, "ACGTNacgtRY")]
    bs = make_set(reads, haps, seed=12)
    assert_close(forward_host(bs), O.phmm_oracle(bs))


def test_prior_tables_against_compares(monkeypatch):
    """GBX_PHMM_LUT=0 is round 5's compare-and-select form of the stream kernels: same sums, bit for bit (the table holds the
    two values the select chose between)."""
    bs = gen_phmm(30, 3003)
    a = forward_host(bs)
    monkeypatch.setenv("GBX_PHMM_LUT", "0")
    b = forward_host(bs)
    assert np.array_equal(a, b)
    assert_close(a, O.phmm_oracle(bs, 8, True)[0])


def test_device_entry_and_batch_subset_equivalence():
    import torch
    bs = gen_phmm(30, 11)
    d = DevicePhmmBatchSet(bs, torch.device("cuda:0"))
    s = torch.cuda.current_stream().cuda_stream
    d.run(s)
    torch.cuda.synchronize()
    full = d.results().copy()
    d.out.fill_(0)
    d.run(s)
    torch.cuda.synchronize()
    assert np.array_equal(d.results(), full)              # deterministic: no atomics on the data path
    assert_close(full, O.phmm_oracle(bs, 8))
    part = forward_host(bs.take_batches(10, 20))
    lo, hi = int(bs.batch_pair_off[10]), int(bs.batch_pair_off[20])
    assert np.array_equal(part, full[lo:hi])              # sharding by whole batches changes nothing


def test_host_entry_staged_transfers(monkeypatch):
    """Staged host path (pinned slabs, upload workers, downloader) against the oracle; see test_chain_gpu."""
    bs = gen_phmm(30, 515)
    want, _ = O.phmm_oracle(bs, 8, True)
    monkeypatch.setenv("GBX_HOST_STAGE_MIN", "0")
    assert_close(forward_host(bs), want)
    monkeypatch.setenv("GBX_HOST_PAGEABLE", "1")
    assert_close(forward_host(bs), want)


def test_one_long_haplotype_does_not_size_every_pair():
    """A 30 000-base haplotype among ordinary ones: the host entry sizes the haplotype streams by the exact sum over
    the pairs of haplen+1 (here 28 MB: every read meets the long haplotype once) instead of n_pairs x (longest+1)
    (216 MB); results as the oracle's."""
    rng = np.random.default_rng(17)
    haps = [rand_seq(rng, int(rng.integers(150, 320))) for _ in range(7)] + [rand_seq(rng, 30000)]
    reads = [haps[int(rng.integers(0, 7))][:int(rng.integers(40, 140))] for _ in range(900)]
    reads.append(haps[7][1000:1151])
    bs = make_set(reads, haps, seed=3)
    from genomicsbench_amd import _native as N
    exact = int((bs.hap_len[bs.pair_hap].astype(np.int64) + 1).sum())
    assert exact < bs.n_pairs * 30001 // 5
    assert_close(forward_host(bs), O.phmm_oracle(bs, 8))
