"""CPU-side checks for whole-seed extension: the restatement on hand-worked seeds and against the compiled reference, the
generator, and the host entry's argument checks (which run before any device is touched)."""
import numpy as np
import pytest

from genomicsbench_amd import _native as N
from genomicsbench_amd.bsw_seeds import SEED_DTYPE, SeedBatch, extend_seeds_host, gen_seeds, make_seed_params
from oracle import oracle_py as O
import seedext_ref as R

A = lambda *x: np.array(x, dtype=np.uint8)
F = {f: k for k, f in enumerate(("score", "truesc", "qb", "qe", "rb", "re", "w", "sc0"))}


def one(read, win, qbeg, rbeg, ln, **kw):
    b = SeedBatch.from_reads([np.asarray(read, np.uint8)], [np.asarray(win, np.uint8)], [qbeg], [rbeg], [ln])
    st = {}
    o = R.extend_seeds_ref(make_seed_params(**kw), b, stats=st)[0]
    return {f: int(o[k]) for f, k in F.items()}, st


def test_exact_match_read_extends_end_to_end():
    rng = np.random.default_rng(1)
    read = rng.integers(0, 4, 60).astype(np.uint8)
    win = np.concatenate([rng.integers(0, 4, 7), read, rng.integers(0, 4, 9)]).astype(np.uint8)
    o, st = one(read, win, 20, 27, 15)
    assert (o["qb"], o["qe"], o["truesc"]) == (0, 60, 60)
    assert o["rb"] == 27 - 20 and o["re"] == 7 + 60
    assert o["sc0"] == 35 and o["score"] == 60 and o["w"] == 100
    assert [x["pairs"] for x in st["left"]] == [1] and [x["pairs"] for x in st["right"]] == [1]


def test_seed_at_read_start_has_no_left_phase():
    read = A(0, 1, 2, 3, 0, 1, 2, 3, 3, 2)
    o, st = one(read, np.concatenate([read, A(1, 1)]), 0, 0, 4)
    assert "left" not in st and o["qb"] == 0 and o["rb"] == 0 and o["sc0"] == 4
    assert (o["qe"], o["re"], o["truesc"], o["score"]) == (10, 10, 10, 10)


def test_seed_ending_at_read_end_has_no_right_phase():
    read = A(2, 2, 0, 1, 3, 0, 1, 2)
    o, st = one(read, np.concatenate([A(3), read]), 4, 5, 4)
    assert "right" not in st and o["qe"] == 8 and o["re"] == 5 + 4
    assert (o["qb"], o["rb"], o["truesc"], o["score"], o["sc0"]) == (0, 1, 8, 8, 8)


def test_mismatching_tail_beyond_pen_clip_is_local():
    rng = np.random.default_rng(3)
    core = rng.integers(0, 4, 40).astype(np.uint8)
    tail = rng.integers(0, 4, 12).astype(np.uint8)
    read = np.concatenate([core, tail])
    win = np.concatenate([core, (tail + 1) % 4])            # every tail base mismatches: the to-end score is far below
    o, st = one(read, win, 0, 0, 20)
    assert (o["qe"], o["re"], o["truesc"], o["score"]) == (40, 40, 40, 40)
    # the same with a pen_clip3 large enough to pay for the mismatches: to-end
    o2, _ = one(read, win, 0, 0, 20, pen_clip3=100)
    assert o2["qe"] == 52 and 0 < o2["truesc"] < 40 - 5


@pytest.mark.skipif(O.ref_lib("bsw") is None, reason="compiled reference only exists in the build container")
def test_restatement_ksw_steps_match_compiled_reference():
    """Every ksw step the restatement makes (both sides, every try, band retries on) equals scalarBandedSWA of the
    reference's own bandedSWA.cpp."""
    b = gen_seeds(3000, 11, indel_rate=0.5, max_indel=8)
    calls = []

    def ksw(params, pb):
        want = O.bsw_ref_scalar(params, pb)
        got = O.bsw_oracle(params, pb, 4)
        assert np.array_equal(got, want)
        calls.append((params.w, pb.n))
        return got
    R.extend_seeds_ref(make_seed_params(w=5, max_band_try=3), b, ksw=ksw)
    assert {5, 10} <= {w for w, _ in calls} and len(calls) >= 3


def test_generator_is_deterministic_and_seeds_match_exactly():
    a, b = gen_seeds(5000, 7), gen_seeds(5000, 7)
    assert np.array_equal(a.ref, b.ref) and np.array_equal(a.qer, b.qer) and np.array_equal(a.seeds, b.seeds)
    assert not np.array_equal(gen_seeds(5000, 8).qer, a.qer)
    s = a.seeds
    for k in range(a.n):
        q = a.qer[s["qoff"][k] + s["qbeg"][k]:][:s["len"][k]]
        r = a.ref[s["roff"][k] + s["rbeg"][k]:][:s["len"][k]]
        assert np.array_equal(q, r)
    assert (s["rbeg"] < s["qbeg"]).any() and ((s["rbeg"] == 0) & (s["qbeg"] > 0)).any()
    assert (s["qbeg"] == 0).any() and (s["qbeg"] + s["len"] == s["lq"]).any()
    assert (np.bincount(s["lq"]).argmax() == 151) and (s["lq"] > 1000).any()
    assert (a.qer == 4).any()


def _seeds_case():
    return gen_seeds(50, 3)


BAD = [
    ("qbeg", -1), ("len", 0), ("qbeg+len>lq", None), ("rbeg", -1), ("rbeg+len>rlen", None),
    ("qoff", -1), ("roff", -1), ("qoff past arena", None), ("roff past arena", None),
]


@pytest.mark.parametrize("what,val", BAD, ids=[w for w, _ in BAD])
def test_host_entry_rejects_malformed_seed_naming_it(what, val):
    b = _seeds_case()
    s = b.seeds.copy()
    k = 17
    if what == "qbeg+len>lq":
        s["qbeg"][k] = s["lq"][k] - s["len"][k] + 1
    elif what == "rbeg+len>rlen":
        s["rbeg"][k] = s["rlen"][k] - s["len"][k] + 1
    elif what == "qoff past arena":
        s["qoff"][k] = b.qer.size - s["lq"][k] + 1
    elif what == "roff past arena":
        s["roff"][k] = b.ref.size - s["rlen"][k] + 1
    else:
        s[what][k] = val
    s["qbeg"][k + 5] = -7                                 # a later bad seed: the lowest one is named
    with pytest.raises(N.GbxError) as e:
        extend_seeds_host(make_seed_params(), SeedBatch(b.ref, b.qer, s))
    assert e.value.code == N.GBX_ERR_ARG and "seed 17 " in str(e.value)


def test_host_entry_rejects_sides_beyond_limits():
    read = np.zeros(9000, np.uint8)
    b = SeedBatch.from_reads([read], [read], [8500], [8500], [20])       # left query 8 500 > GBX_BSW_MAX_QLEN
    with pytest.raises(N.GbxError) as e:
        extend_seeds_host(make_seed_params(), b)
    assert e.value.code == N.GBX_ERR_UNSUPPORTED and "seed 0" in str(e.value)


@pytest.mark.parametrize("mbt", [0, 5])
def test_host_entry_rejects_max_band_try(mbt):
    with pytest.raises(N.GbxError) as e:
        extend_seeds_host(make_seed_params(max_band_try=mbt), _seeds_case())
    assert e.value.code == N.GBX_ERR_ARG and "max_band_try" in str(e.value)


def test_abi_layout():
    from genomicsbench_amd.bsw_seeds import SeedParams, lib
    import ctypes as C
    assert SEED_DTYPE.itemsize == 40 and C.sizeof(SeedParams) == C.sizeof(N.BswParams) + 16
    p = make_seed_params()
    assert (p.pen_clip5, p.pen_clip3, p.max_band_try, p.bsw.w, p.bsw.mat[0]) == (5, 5, 2, 100, 1)
    assert lib().gbx_bsw_seeds_workspace_bytes(1000, 10000, 5000) >= 1000 * 136 + 15000
    # n = 0 is fine and touches nothing
    assert extend_seeds_host(p, SeedBatch(np.zeros(4, np.uint8), np.zeros(4, np.uint8), np.zeros(0, SEED_DTYPE))).shape == (0, 8)
