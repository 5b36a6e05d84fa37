"""The CIGAR stage without a GPU: the restated rules (tests/mem_cigar_ref.py) in their two forms and the C twin on the hand-built
cases, invariants that rest on no one's memory of bwa, the frozen worked example, the exported symbols, and the argument checks
of the host entry that come before a device is touched."""
import ctypes as C
import functools

import numpy as np
import pytest

from genomicsbench_amd import _native as N
from genomicsbench_amd import mem_cigar as MG
from genomicsbench_amd.bsw_seeds import SEED_DTYPE
import mem_cigar_cases as K
import mem_cigar_ref as R


@pytest.fixture(scope="module")
def refs():
    return {name: K.reference(j) for name, j in K.hand_built().items()}


def by_name(j, out, name):
    k = j["names"].index(name)
    return out[0][k], K.cigar_of(out[0], out[1], k)


def test_both_lookups_and_the_c_twin_agree(refs):
    for name, j in K.hand_built().items():
        K.same(K.reference(j, R.global_full), refs[name])
        K.same(K.reference_c(j), refs[name])
    for seed, kw in ((3, {}), (4, dict(a=2, b=3, o_del=5, e_del=2, o_ins=4, e_ins=1)), (5, dict(w=3))):
        j = K.synthetic(24, seed, read_len=(30, 90), **kw)
        want = K.reference(j)
        K.same(K.reference(j, R.global_full), want)
        K.same(K.reference_c(j), want)
        assert (want[0]["rid"] >= 0).sum() > 15 and (want[0]["rid"] < 0).any()


def test_invariants_of_every_case(refs):
    for name, j in K.hand_built().items():
        K.check_invariants(j, *refs[name])
    j = K.synthetic(40, 3)
    K.check_invariants(j, *K.reference_c(j))


def test_worked_example_from_its_fixture():
    ex = K.example()
    g = np.array([int(c) for c in ex["genome"]], dtype=np.uint8)
    qer = np.array([int(c) for r in ex["reads"] for c in r], dtype=np.uint8)
    seeds, res = np.zeros(2, dtype=R.SEED_DTYPE), np.zeros(2, dtype=R.RESULT_DTYPE)
    for k in range(2):
        for f, v in ex["seeds"][k].items():
            seeds[k][f] = v
        for f, v in ex["results"][k].items():
            res[k][f] = v
    for lookup in (R.global_rolling, R.global_full):
        alns, cigar = R.run(R.params(), seeds, res, K.text_of(g), qer, len(g), ex["contig_off"], lookup)
        for k in range(2):
            assert {f: int(alns[k][f]) for f in ex["alns"][k]} == ex["alns"][k]
            assert K.cigar_of(alns, cigar, k) == ex["cigars"][k]
    assert ex["cigars"] == ["2S6M1D9M", "7M1I7M3S"]


def test_the_cases_are_what_their_names_say(refs):
    J = K.hand_built()
    a, c = by_name(J["simple"], refs["simple"], "perfect")
    assert c == "50M" and a["w"] == 0 and a["nm"] == 0 and a["score"] == 50            # the path without a DP
    a, c = by_name(J["simple"], refs["simple"], "three_mismatches")
    assert c == "50M" and a["w"] > 0 and a["nm"] == 3                                   # the same lengths through the DP
    assert by_name(J["simple"], refs["simple"], "an_N")[0]["score"] == 48
    # an indel in a homopolymer lands leftmost on the forward strand, whichever strand the read is on
    for kind, want in (("del", "20M1D29M"), ("ins", "20M1I30M")):
        f, r = (by_name(J["strand"], refs["strand"], "homopolymer_%s_%s" % (kind, s)) for s in ("fwd", "rev"))
        assert f[1] == r[1] == want and f[0]["pos"] == r[0]["pos"] == 480 and (f[0]["is_rev"], r[0]["is_rev"]) == (0, 1)
    assert by_name(J["strand"], refs["strand"], "clips_fwd")[1] == by_name(J["strand"], refs["strand"], "clips_rev")[1] == "5S39M1D20M7S"
    for name in ("crosses_L", "all_minus_one", "empty_query", "empty_text"):
        a, c = by_name(J["strand"], refs["strand"], name)
        assert a["rid"] == -1 and c == "" and a["pos"] == 0 and a["n_cigar"] == 0
    # a deletion at either end: the position moves for the leading one only, and nm does not count it
    for s in ("_fwd", "_rev"):
        a, c = by_name(J["squeeze"], refs["squeeze"], "leading_deletion" + s)
        assert (c, a["pos"], a["nm"], a["score"]) == ("45M", 105, 0, 34)
        a, c = by_name(J["squeeze"], refs["squeeze"], "trailing_deletion" + s)
        assert (c, a["pos"], a["nm"], a["score"]) == ("45M", 100, 0, 34)
        a, c = by_name(J["squeeze"], refs["squeeze"], "both_ends" + s)             # only the leading one goes
        assert (c, a["pos"], a["nm"]) == ("40M5D", 105, 0)
    T = lambda name, job="tries": by_name(J[job], refs[job], name)[0]
    assert (T("band_doubles_twice")["tries"], T("band_doubles_twice")["w"]) == (3, 8)
    assert (T("capped_by_the_results_w")["tries"], T("capped_by_the_results_w")["w"]) == (2, 10)       # min(w2, r.w) = 5, doubled once
    assert (T("not_capped")["tries"], T("not_capped")["w"]) == (1, 16)                                 # r.w above w2: 4 w
    assert T("same_score_stops")["tries"] == 2 and T("same_score_stops_dp")["tries"] == 2
    assert (T("stops_at_4w", "tries_4w")["tries"], T("stops_at_4w", "tries_4w")["w"]) == (1, 4)
    assert T("w_zero_gap", "tries_w0")["tries"] == 1
    a, c = by_name(J["band_and_strips"], refs["band_and_strips"], "narrow_band_60")
    assert 2 * R.band(R.params(), 60, 60, int(a["w"])) + 1 < 60
    a, c = by_name(J["band_and_strips"], refs["band_and_strips"], "band_wider_than_a_strip")
    assert R.band(R.params(), 127, 210, int(a["w"])) > 64


def test_the_tie_cases_hit_every_tie():
    j = K.hand_built()["ties"]
    seen = set()
    R.run(K.p_of(j), j["seeds"], j["res"], j["text"], j["qer"], j["L"], j["contig_off"], functools.partial(R.global_rolling, events=seen))
    assert seen >= {"m==e", "h==f", "e==t", "f==t"}


def test_new_symbols_are_exported():
    L = N.lib()
    for name in ("gbx_mem_cigar_default_params", "gbx_mem_cigar_record_z_bytes", "gbx_mem_cigar_workspace_bytes", "gbx_mem_cigar_device",
                 "gbx_mem_cigar_host"):
        assert hasattr(L, name), name
    p = MG.make_params()
    assert list(p.mat) == R.DEFAULTS["mat"] and {k: getattr(p, k) for k in ("o_del", "e_del", "o_ins", "e_ins", "w")} == \
        {k: R.DEFAULTS[k] for k in ("o_del", "e_del", "o_ins", "e_ins", "w")}
    assert list(MG.make_params(a=2, b=3).mat) == R.scmat(2, 3)
    assert C.sizeof(MG.CigarParams) == 120 and MG.ALN_DTYPE == R.ALN_DTYPE and MG.ALN_DTYPE.itemsize == 48
    assert MG.RESULT_DTYPE == R.RESULT_DTYPE and SEED_DTYPE == R.SEED_DTYPE
    z = MG.lib().gbx_mem_cigar_record_z_bytes(C.byref(p), 151, 160)
    assert 151 * 23 < z < 4 * 151 * 160
    assert MG.lib().gbx_mem_cigar_workspace_bytes(1000, 1 << 20) >= (1 << 20) + 1000 * 16
    with pytest.raises(TypeError):
        MG.make_params(zdrop=100)
    assert MG.cigar_string(np.array([5 << 4 | 4, 96 << 4, 1 << 4 | 2, 50 << 4 | 0, 2 << 4 | 1], np.uint32)) == "5S96M1D50M2I"


def host_rc(j, **kw):
    p = MG.make_params(**dict(j["params"], **kw.pop("params", {})))
    j = dict(j, **kw)
    try:
        MG.cigar_host(p, j["seeds"], j["res"], j["text"], j["qer"], j["L"], j["contig_off"])
    except N.GbxError as e:
        return e.code, str(e)
    return 0, ""


def test_host_entry_checks_its_arguments_before_a_device_is_touched():
    """GBX_ERR_ARG (-1), not GBX_ERR_NO_DEVICE: these returns come before the first HIP call."""
    j = K.hand_built()["strand"]
    rc, msg = host_rc(j, params=dict(e_del=0))
    assert rc == N.GBX_ERR_ARG and "e_del" in msg
    assert host_rc(j, params=dict(e_ins=0))[0] == N.GBX_ERR_ARG
    rc, msg = host_rc(j, params=dict(w=-1))
    assert rc == N.GBX_ERR_ARG and "w" in msg
    rc, msg = host_rc(j, contig_off=np.array([0, 900, 700, 1600], dtype=np.int64))
    assert rc == N.GBX_ERR_ARG and "contig_off" in msg
    assert host_rc(j, contig_off=np.array([0, 700, 1599], dtype=np.int64))[0] == N.GBX_ERR_ARG
    assert host_rc(j, contig_off=np.array([1, 700, 1600], dtype=np.int64))[0] == N.GBX_ERR_ARG

    def record(k, res_field=None, seed_field=None, value=0):
        seeds, res = j["seeds"].copy(), j["res"].copy()
        if res_field:
            res.view(R.RESULT_DTYPE).reshape(-1)[k][res_field] = value
        if seed_field:
            seeds[k][seed_field] = value
        return host_rc(j, seeds=seeds, res=res)
    rc, msg = record(2, res_field="qe", value=10_000)                   # past the read
    assert rc == N.GBX_ERR_ARG and "record 2" in msg
    rc, msg = record(1, seed_field="qoff", value=len(j["qer"]) - 3)     # the read leaves the arena
    assert rc == N.GBX_ERR_ARG and "record 1" in msg
    assert record(3, seed_field="qoff", value=-1)[0] == N.GBX_ERR_ARG
    assert record(0, seed_field="roff", value=-100)[0] == N.GBX_ERR_ARG
    rc, msg = record(7, res_field="re", value=100_000)                  # reverse strand, past 2 L
    assert rc == N.GBX_ERR_ARG and "record 7" in msg
    rc, msg = host_rc(j, text=j["text"][:2000])                         # the text shorter than a region needs
    assert rc == N.GBX_ERR_ARG and "record" in msg
