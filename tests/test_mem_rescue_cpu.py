"""The restated mate-rescue rules (tests/mem_rescue_ref.py) against hand-built cases with the outcome written out, the frozen
example, and the conditions the GPU test relies on: no boundary input in any committed case or generated GPU input, and the new
mapq and decision rules equal to the existing ones where csub = 0 and seedlen0 >= 1."""
import numpy as np
import pytest

import mem_pair_cases as KP
import mem_pair_ref as PR
import mem_regs_ref as RG
import mem_rescue_cases as K
import mem_rescue_ref as R


@pytest.mark.parametrize("name", sorted(K.sw_cases()))
def test_hand_built_sw(name):
    q, t, P, want = K.sw_cases()[name]
    assert R.sw(q, t, R.params(**P)) == want


def test_sw_widths_and_padding():
    P = R.params()
    assert [R.lanes_of(m, P) for m in (1, 249, 250, 1024)] == [16, 16, 8, 8]
    assert R.lanes_of(49, R.params(a=5)) == 16 and R.lanes_of(50, R.params(a=5)) == 8


def test_the_run_rule_makes_a_second_entry():
    """The entry of a run stays at the column of its maximum, so the column two behind it starts another."""
    q, t, P, _ = K.sw_cases()["run_second_entry"]
    _, te, _, ents = R.sw_pass(np.asarray(q, np.int64), np.asarray(t, np.int64), R.params(**P), 16)
    assert te == 36 and ents == [(32, 36), (24, 38), (22, 40), (20, 42)]


def test_padded_rows_change_score2():
    """The same sub-hit without the padded rows' reach (one column fewer behind it) has no second entry."""
    q, t, P, _ = K.sw_cases()["pad_reach"]
    ents = R.sw_pass(np.asarray(q, np.int64), np.asarray(t, np.int64), R.params(**P), 16)[3]
    carried = [(20, 24 + 2 * k) for k in range(7)]    # the hit itself, carried on by the 12 padded rows
    assert ents == carried + [(19, 44), (19, 46)]
    ents = R.sw_pass(np.asarray(q, np.int64), np.asarray(K.sw_cases()["pad_cut"][1], np.int64), R.params(**P), 16)[3]
    assert ents == carried + [(19, 44)]


def test_sw_against_a_plain_matrix():
    """Score and end of the vectorised pass against the recurrence written cell by cell, on random inputs with gaps."""
    rng = np.random.default_rng(5)
    P = R.params(min_seed_len=4)
    for _ in range(20):
        m, n = int(rng.integers(1, 40)), int(rng.integers(1, 60))
        q, t = rng.integers(0, 5, m), rng.integers(0, 4, n)
        if m > 12 and n > 20:
            t[5:5 + m - 3] = np.delete(q, [4, 5, 6])[:len(t[5:5 + m - 3])]
        Pw = R.lanes_of(m, P)
        mp = (m + Pw - 1) // Pw * Pw
        qq = list(q) + [R.PAD] * (mp - m)
        H = np.zeros((n + 1, mp + 1), dtype=np.int64)
        E = np.zeros((n + 2, mp + 1), dtype=np.int64)
        best = (0, -1)
        for i in range(n):
            F = 0
            for j in range(mp):
                s = 0 if qq[j] == R.PAD else -1 if qq[j] > 3 or t[i] > 3 else P["a"] if qq[j] == t[i] else -P["b"]
                h = max(0, H[i, j] + s, E[i, j + 1], F)
                H[i + 1, j + 1] = h
                E[i + 1, j + 1] = max(0, E[i, j + 1] - P["e_del"], h - P["o_del"] - P["e_del"])
                F = max(0, F - P["e_ins"], h - P["o_ins"] - P["e_ins"])
            if H[i + 1].max() > best[0]:
                best = (int(H[i + 1].max()), i)
        got = R.sw_pass(np.asarray(q, np.int64), np.asarray(t, np.int64), P, Pw)
        assert (got[0], got[1]) == best


@pytest.mark.parametrize("name", sorted(K.hand_built()))
def test_hand_built_calls(name):
    j = K.hand_built()[name]
    w = K.reference(j)
    assert [tuple(int(v) for v in x)[:3] for x in w["stats"]] == j["expect"]
    resc = [tuple(int(x[f]) for f in ("read", "rb", "re", "qb", "qe", "score", "csub")) for x in w["xregs"] if x["seedlen0"] == 0]
    assert resc == j["rescued"]
    for x in w["xregs"][w["xregs"]["seedlen0"] == 0]:
        s = w["xseeds"][int(x["seed"])]
        assert int(x["seed"]) >= len(j["seeds"]) and s["len"] == 0 and s["roff"] <= x["rb"] and x["re"] <= s["roff"] + s["rlen"]
        assert s["qbeg"] == x["qb"] and s["roff"] + s["rbeg"] == x["rb"] and s["lq"] == j["read_len"][int(x["read"])]
        assert x["truesc"] == 0 and x["w"] == 0 and x["seedcov"] == min(x["re"] - x["rb"], x["qe"] - x["qb"]) >> 1


def test_is_rev_coordinates():
    """A rescued region on the reverse strand covers the mate's bases: the text there is the read."""
    for name in ("directions", "clamp_2L", "contig_edge"):
        j = K.hand_built()[name]
        w = K.reference(j)
        for x in w["xregs"][w["xregs"]["seedlen0"] == 0]:
            rd = j["qer"][int(j["read_off"][x["read"]]):][:int(j["read_len"][x["read"]])]
            assert np.array_equal(j["text"][int(x["rb"]):int(x["re"])], rd[int(x["qb"]):int(x["qe"])])


def test_a_pair_that_needs_nothing_is_byte_equal():
    for name, pairs in (("needs_nothing", [0]), ("contig_edge", [1]), ("window_18_19", [0])):
        j = K.hand_built()[name]
        w = K.reference(j)
        for p in pairs:
            a, b = int(j["reg_off"][2 * p]), int(j["reg_off"][2 * p + 2])
            x = w["xregs"][int(w["xreg_off"][2 * p]):int(w["xreg_off"][2 * p + 2])].copy()
            y = j["regs"][a:b].copy()
            x["sel"], y["sel"] = 0, 0                 # the index in the list depends on the pairs before it
            assert x.tobytes() == y.tobytes()


def test_the_knocked_out_original_is_gone():
    j = K.hand_built()["knocks_out_original"]
    w = K.reference(j)
    mate = w["xregs"][int(w["xreg_off"][1]):int(w["xreg_off"][2])]
    assert len(mate) == 1 and mate[0]["seedlen0"] == 0 and mate[0]["score"] == 50 and len(j["regs"]) == 2


def test_frozen_example():
    ex = K.example()
    j = K.hand_built()[ex["job"]]
    w = K.reference(j)
    assert [[int(v) for v in x] for x in w["xregs"].tolist()] == ex["xregs"]
    assert [[int(v) for v in x] for x in w["stats"].tolist()] == ex["stats"]
    assert [[int(v) for v in x] for x in w["xseeds"][len(j["seeds"]):].tolist()] == ex["new_seeds"]
    assert w["xsel_res"][:w["n_xsel"]].tolist() == ex["xsel_res"]


def test_no_boundary_inputs():
    """A condition of the GPU test: with no boundary input a device log() that differs in the last bit cannot change a byte."""
    for name, j in list(K.hand_built().items()) + list(K.gpu_inputs().items()):
        assert K.reference(j)["boundary"] == 0, name
    for name, (q, t, P, _) in K.sw_cases().items():
        assert K.reference(K.sw_job(q, t, P))["boundary"] == 0, name


def test_generated_inputs_are_what_they_claim():
    w = K.reference(K.gpu_inputs()["many"])
    active = int((w["stats"]["n_sw"] > 0).sum())
    assert 70 <= active <= 140 and w["stats"]["n_kept"].sum() >= 60
    j = K.gpu_inputs()["many_regions"]
    assert int(j["reg_off"][2] - j["reg_off"][1]) == 70 and K.reference(j)["stats"]["n_kept"][0] == 1
    assert K.reference(K.gpu_inputs()["wide_window"])["stats"].tolist() == [(1, 1, 1, 0)]


def test_unchanged_callers():
    """With csub = 0 and seedlen0 >= 1 the new mapq and decision rules are the existing ones, on every region of the paired
    stage's GPU inputs."""
    n = 0
    for j in KP.gpu_inputs().values():
        Pp = KP.p_of(j)
        Pr = R.params(**{k: v for k, v in Pp.items() if k in R.DEFAULTS})
        Pg = RG.params(**{k: v for k, v in Pp.items() if k in RG.DEFAULTS})
        for row in j["regs"][:400]:
            x = R.Reg(row.view(R.REG_DTYPE))
            assert x.csub == 0 and x.seedlen0 >= 1
            x.lq = int(j["seeds"][x.seed]["lq"])
            l_rep = int(j["l_rep"][x.read])
            old = PR.Reg(row)
            old.lq = x.lq
            assert R.mapq_values(x, l_rep, Pr) == RG.mapq_values(old, l_rep, Pg)
            assert R.mapq_se(x, l_rep, Pr) == PR.mapq_se(old, l_rep, x.lq, Pp, PR.Boundary())
            assert R.decision_cap(x, Pr) == PR.raw_mapq(x.score, Pp, PR.Boundary())
            assert float(R.frac_rep_of(x, l_rep)) == float(np.float32(l_rep) / np.float32(x.lq))
            n += 1
    assert n > 1000
