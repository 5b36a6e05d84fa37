"""meth-freq on the device against the Python restatement of freq.c (tests/abea_freq_ref.py) and the compiled reference's recorded
outputs (tests/golden/abea_freq_reference.json).  Every comparison is exact: bytes and integers."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abea_freq_cases as K  # noqa: E402
import abea_freq_ref as R  # noqa: E402
from genomicsbench_amd import _native as N  # noqa: E402
from genomicsbench_amd import abea_freq as AF  # noqa: E402
from genomicsbench_amd import abea_meth as AM  # noqa: E402
from genomicsbench_amd.abea import PAIR_DTYPE  # noqa: E402
from test_abea_freq_cpu import DRIVER, golden_cases  # noqa: E402

pytestmark = pytest.mark.gpu
METH_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "abea_meth.npz")
CANARY = 0xA5
SIZES = [0, 1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097]        # the wavefront, the scan block, the sort tile


def device():
    import torch
    return torch.device("cuda:0")


def on_device(rec, arena, names, thr=2.5, split=False, pos_bits=31, contig_bits=None):
    """records -> DeviceAbeaFreq, filled"""
    d = AF.DeviceAbeaFreq(device(), thr, split, pos_bits, contig_bits or AF.bits_for(max(len(names) - 1, 1)))
    d.add_records(rec, arena)
    d.count()
    d.size()
    d.fill()
    return d


def check_rows(rows, thr=2.5, split=False, pos_bits=31, host=True):
    """the device entry (and the host entry) on `rows` against the restatement: the table and the text"""
    rec, arena, names = K.to_records(rows)
    want = R.table(K.ref_records(rows), thr, split)
    d = on_device(rec, arena, names, thr, split, pos_bits)
    sites, seqs = d.results()
    assert K.table_rows(sites, seqs, names) == want
    assert d.n_sites == len(want) and not sites["pad_"].any()
    assert d.text(names) == R.text_of(want)
    if host:
        hs, ha = AF.freq_host(rec, arena, thr, split)
        assert hs.tobytes() == sites.tobytes() and ha.tobytes() == seqs.tobytes()
    return d, want


# ------------------------------------------------------------------------------------------------ golden
@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c[0])
def test_golden_through_the_device_the_host_entry_and_the_driver(case, tmp_path):
    name, text, thr, split, kind, want = case
    rec, arena, names, got_kind = AF.parse_tsv(text)
    assert got_kind == kind
    d = on_device(rec, arena, names, thr, split)
    assert d.text(names, kind) == want
    sites, seqs = d.results()
    assert R.text_of(K.table_rows(sites, seqs, names), kind) == want
    hs, ha = AF.freq_host(rec, arena, thr, split)
    assert hs.tobytes() == sites.tobytes() and ha.tobytes() == seqs.tobytes()
    assert AF.tsv_host(hs, ha, names, kind) == want
    assert AF.tsv_host(hs, ha, names, kind, with_header=False) == want[len(R.OUT_HEADERS[kind]):]
    src, dst = tmp_path / "in.tsv", tmp_path / "out.tsv"
    src.write_bytes(text)
    opts = (["-s"] if split else []) + (["-c", repr(thr)] if thr != 2.5 else [])
    r = subprocess.run([DRIVER] + opts, input=text, capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stdout == want, r.stderr[-2000:]
    r = subprocess.run([DRIVER, "-i", str(src), "-o", str(dst)] + opts, capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stdout == b"" and dst.read_bytes() == want, r.stderr[-2000:]


# ------------------------------------------------------------------------------------------------ sizes
@pytest.mark.parametrize("n", SIZES)
def test_sizes(n):
    rows = K.random_rows(100 + n, n, n // 5 + 1)
    check_rows(rows, 2.5, False)
    check_rows(rows, 1.0, True, host=False)
    check_rows(K.random_rows(200 + n, n, 0, distinct=True), 0.0, False, pos_bits=24, host=False)       # every key its own segment, three digits a coordinate


def test_one_key_5000_times():
    """a segment longer than a block, a scan block and a sort tile, starting in the last lane of a block: 255 smaller keys before it"""
    for lead in (255, 4095):
        rows = [("chr1", 10 + k, 10 + k, "3.00", 1, "ACGA") for k in range(lead)]
        rows += [("chr1", 100000, 100000, "3.00" if k % 3 else "-3.00", 1 + (k == 0), "TTCGCGAA" if k == 0 else "AACGA") for k in range(5000)]
        rows += [("chr1", 100001, 100001, "-3.00", 1, "ACGA"), ("chr2", 5, 5, "3.00", 1, "ACGA")]
        order = np.random.default_rng(lead).permutation(len(rows) - 1) + 1                    # the first-seen record stays first
        rows = [rows[0]] + [rows[k] for k in order]
        first = next(r for r in rows if r[1] == 100000)
        d, want = check_rows(rows)
        big = [w for w in want if w[1] == 100000][0]
        assert big[4] == 5001 and big[3] == first[4] and big[6] == first[5].encode()
        assert want.index(big) == lead


# ------------------------------------------------------------------------------------------------ keys
def test_key_range():
    rows = []
    for c in range(300):                                                                      # a second radix digit for the contig
        rows.append(("ctg%03d" % (299 - c), K.INT_MAX if c % 7 == 0 else c, K.INT_MAX if c % 7 == 0 else c + 1, "3.00", 1, "ACG"))
        rows.append(("ctg%03d" % (299 - c), 5, 5 + c % 3, "-3.00", 2, "ACGCG"))
    rows += [("chr10", 4, 4, "3.00", 1, "ACG"), ("chr2", 4, 4, "3.00", 1, "ACG"), ("chr2", 4, 9, "3.00", 1, "ACG"), ("chr2", 4, 6, "3.00", 1, "ACG"),
             ("chr2", 3, K.INT_MAX, "3.00", 1, "ACG"), ("chr2", K.INT_MAX, 0, "3.00", 1, "ACG")]
    d, want = check_rows(rows)
    names = [w[0] for w in want]
    assert names.index(b"chr10") < names.index(b"chr2") and len(set(names)) == 302
    assert [w[2] for w in want if w[0] == b"chr2" and w[1] == 4] == [4, 6, 9]
    check_rows(rows, split=True, host=False)


def test_key_bits_too_few_are_flagged():
    rec, arena, names = K.to_records([("chr1", 300, 300, "3.00", 1, "ACG"), ("chr1", 2, 2, "3.00", 1, "ACG")])
    d = AF.DeviceAbeaFreq(device(), 2.5, False, pos_bits=8, contig_bits=1)
    d.add_records(rec, arena)
    d.count()
    with pytest.raises(N.GbxError) as e:
        d.size()
    assert e.value.code == N.GBX_ERR_ARG and d.flags == AF.KEY_BITS


# ------------------------------------------------------------------------------------------------ calls
def test_calls():
    below = [("chr1", k, k, "2.49" if k & 1 else "-1.00", 1, "ACG") for k in range(70)]
    d, want = check_rows(below)
    assert want == [] and d.n_sites == 0 and d.text(["chr1"]) == R.OUT_HEADERS[1] and d.text(["chr1"], AF.MOTIFS) == R.OUT_HEADERS[2]
    zero = [("chr1", 5, 5, "0.00", 0, "AAA"), ("chr1", 6, 6, "0.00", 0, "CCC"), ("chr1", 6, 6, "0.50", 3, "CGCGCG"), ("chr1", 7, 7, "-0.00", 1, "ACG")]
    d, want = check_rows(zero, thr=0.0)
    assert want == [(b"chr1", 6, 6, 0, 3, 3, b"CCC"), (b"chr1", 7, 7, 1, 1, 0, b"ACG")]
    odd = [("chr1", 5, 5, "nan", 1, "ACG"), ("chr1", 5, 5, "inf", 2, "ACG"), ("chr1", 5, 5, "-inf", 4, "ACG"), ("chr1", 6, 6, "-nan", 1, "ACG")]
    d, want = check_rows(odd, thr=1e300)
    assert want == [(b"chr1", 5, 5, 1, 7, 2, b"ACG"), (b"chr1", 6, 6, 1, 1, 0, b"ACG")]
    check_rows(K.edge_rows(), thr=float("nan"))                                               # fabs(llr) < NaN is false: every record is called


# ------------------------------------------------------------------------------------------------ split
def test_split():
    rows = [("chr1", 10, 20, "6.00", 2, "AAAAAAAA"),                                          # no CG: no item
            ("chr1", 30, 33, "6.00", 2, "CGCG"), ("chr1", 40, 47, "-6.00", 2, "AACGAACG"),    # CGCG; CG as the last two bytes
            ("chr1", 50, 52, "6.00", 2, "AAC"), ("chr1", 60, 62, "6.00", 2, "GAA"),           # C | G across two records of the arena
            ("chr1", 70, 77, "6.00", 2, "aacgAAcg"), ("chr1", 80, 84, "6.00", 2, "cgACG"),    # lowercase is no CG
            ("chr1", 200, 200, "7.00", 1, "GGCGG"), ("chr1", 200, 207, "7.00", 2, "CGTTTTTCG"),
            ("chr1", 300, 309, "-7.00", 2, "ACGTTTTTCG"), ("chr1", 300, 300, "7.00", 1, "TTCGT"),
            ("chr1", 400, 400, "7.00", 5, "C"), ("chr1", 410, 410, "7.00", 5, "G"), ("chr1", 420, 420, "7.00", 5, "")]
    d, want = check_rows(rows, split=True)
    assert (b"chr1", 30, 30, 1, 1, 1, b"split-group") in want and (b"chr1", 32, 32, 1, 1, 1, b"split-group") in want
    assert (b"chr1", 44, 44, 1, 1, 0, b"split-group") in want and (b"chr1", 80, 80, 1, 1, 1, b"split-group") in want
    assert not [w for w in want if 50 <= w[1] < 80 or 400 <= w[1]]
    assert (b"chr1", 200, 200, 1, 2, 2, b"GGCGG") in want and (b"chr1", 300, 300, 1, 2, 1, b"split-group") in want
    rec, arena, names = K.to_records(rows)
    assert arena.tobytes()[rec["seq_off"][4] - 1:rec["seq_off"][4] + 1] == b"CG"                # the pair the scan must not see
    check_rows(K.edge_rows(), split=True)
    check_rows(K.edge_rows(), thr=0.0, split=True)
    big = [("chr1", K.INT_MAX - 2, K.INT_MAX, "3.00", 2, "CGACG")]
    rec, arena, names = K.to_records(big)
    with pytest.raises(N.GbxError) as e:
        AF.freq_host(rec, arena, 2.5, True)
    assert e.value.code == N.GBX_ERR_UNSUPPORTED and "split position" in str(e.value)


# ------------------------------------------------------------------------------------------------ text
def test_text():
    rows = [("c", k, k + 9, "3.00" if k % 4 else "-3.00", 1, "ACG") for k in range(1500)]     # more than a scan block of lines
    rows += [("L" * 255, 0, 0, "3.00", 1, "ACGA"), ("L" * 255, K.INT_MAX, K.INT_MAX, "-3.00", 1000000000, "A" * 200), ("L" * 255, 1000000000, 9, "3.00", 9, "CG")]
    for m, c, pos in ((1, 16, 1), (3, 16, 2), (9, 2000, 3), (5, 2000, 4), (7, 2000, 5), (1999, 2000, 6), (0, 3, 7), (3, 3, 8), (1, 3, 9), (2, 3, 10)):
        rows += [("f", pos, pos, "3.00", m, "ACG"), ("f", pos, pos, "-3.00", c - m, "ACG")]
    d, want = check_rows(rows, thr=0.0)
    text = d.text(sorted({r[0] for r in rows}))
    for f in (b"\t16\t1\t0.062\t", b"\t16\t3\t0.188\t", b"\t2000\t9\t0.004\t", b"\t2000\t5\t0.003\t", b"\t2000\t7\t0.004\t", b"\t2000\t1999\t1.000\t", b"\t3\t0\t0.000\t",
              b"\t3\t3\t1.000\t", b"\t3\t1\t0.333\t", b"\t3\t2\t0.667\t", b"\n" + b"L" * 255 + b"\t2147483647\t2147483647\t1000000000\t1000000000\t0\t0.000\t" + b"A" * 200 + b"\n"):
        assert f in text
    assert text.count(b"\n") == 1 + 1500 + 3 + 10


def test_text_capacity():
    import torch
    rows = K.random_rows(11, 700, 300)
    rec, arena, names = K.to_records(rows)
    d = on_device(rec, arena, names)
    full = d.text(names)
    # the lines that end inside the room are written, the room's end and what lies behind it are not
    lo = np.frombuffer(full, np.uint8)
    ends = np.flatnonzero(lo == 10) + 1
    room = int(ends[len(ends) // 2]) + 3
    nm = [n for n in names]
    off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(n) for n in nm])]).astype(np.int64)).to(d.device)
    arr = torch.from_numpy(np.frombuffer(b"".join(nm) + b"\0" * 16, np.uint8).copy()).to(d.device)
    n = d.n_sites
    work = torch.zeros(int(AF._lib().gbx_abea_freq_tsv_work(n)), dtype=torch.uint8, device=d.device)
    line_off = torch.full((n + 2 + 8,), -7, dtype=torch.int64, device=d.device)
    out = torch.full((len(full) + 64,), CANARY, dtype=torch.uint8, device=d.device)
    call = lambda p, cap: AF._lib().gbx_abea_freq_tsv_device(p, n, d.sites.data_ptr(), d.seq_arena.data_ptr(), len(nm), off.data_ptr(), arr.data_ptr(), AF.CPGS, 1,
                                                             work.data_ptr(), line_off.data_ptr(), cap, out.data_ptr(), None)
    N.check(call(AF.COUNT, 0))
    N.check(call(AF.FILL, room))
    h, lo_h = out.cpu().numpy(), line_off.cpu().numpy()
    assert lo_h[n + 1] == len(full) and (lo_h[n + 2:] == -7).all() and lo_h[0] == 0 and lo_h[1] == len(R.OUT_HEADERS[1])
    kept = int(ends[len(ends) // 2])
    assert h[:kept].tobytes() == full[:kept] and (h[kept:] == CANARY).all()
    hs, ha = d.results()
    with pytest.raises(N.GbxError) as e:
        AF.tsv_host(hs, ha, names, cap=len(full) - 1)
    assert e.value.code == N.GBX_ERR_ARG and str(len(full)) in str(e.value)
    assert AF.tsv_host(hs, ha, names, cap=len(full)) == full


# ------------------------------------------------------------------------------------------------ chained
def _meth_golden():
    g = np.load(METH_GOLDEN)
    ref_off = np.concatenate([[0], np.cumsum(g["ref_len"])[:-1]]).astype(np.int64)
    sites = AM.sites_host(ref_off, g["ref_len"], g["ref_arena"], g["ref_start_pos"], g["rc"], g["rec_off"], g["rec"].copy().view(PAIR_DTYPE).reshape(-1))[0]
    scores = np.stack([g["site_unmeth"].view(np.float32), g["site_meth"].view(np.float32)], axis=1).copy()
    return g, ref_off, sites, scores


@pytest.fixture(scope="module")
def chained():
    g, ref_off, sites, scores = _meth_golden()
    planted = scores.copy()
    for k, diff in enumerate((2.4951171875, -2.4951171875, 2.494140625, 2.125, 2.375, -2.125, -2.375, 0.0048828125, -0.0048828125)):
        for s in range(k, len(sites), 37):
            planted[s] = (-100.0, np.float32(-100.0 + diff))
            assert float(planted[s][1]) - float(planted[s][0]) == diff
    return g, ref_off, sites, scores, planted


@pytest.mark.parametrize("which", ["recorded", "planted"])
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("split", [False, True])
def test_chained_equals_call_methylation_then_meth_freq(chained, which, clip, split):
    g, ref_off, sites, scores, planted = chained
    sc = scores if which == "recorded" else planted
    contigs = ["chr20", "chr20", "chrX", "chr20", "chrM"]
    names = sorted({c.encode() for c in contigs})
    contig_of_read = [names.index(c.encode()) for c in contigs]
    lo, hi = (int(np.sort(sites["start_position"])[40]), int(np.sort(sites["end_position"])[-40])) if clip else (-1, -1)
    tsv = AM.tsv_host(sites, sc, ["read_%d" % r for r in range(5)], contigs, g["rc"], ref_off, g["ref_len"], g["ref_arena"], version=1, clip_start=lo, clip_end=hi,
                      with_header=True)
    for thr in (2.5, 2.12, 0.0):
        want = R.meth_freq(tsv, thr, split)
        assert want.count(b"\n") > 20
        d = AF.DeviceAbeaFreq(device(), thr, split, contig_bits=2)
        d.add_sites(sites, sc.reshape(-1), contig_of_read, ref_off, g["ref_len"], g["ref_arena"], lo, hi)
        d.count()
        d.size()
        d.fill()
        assert d.text(names) == want
    # the host entries, and the records against the parser's reading of the text
    rec, arena = AF.records_host(sites, sc, contig_of_read, ref_off, g["ref_len"], g["ref_arena"], lo, hi)
    prec, parena, pnames, kind = AF.parse_tsv(tsv)
    assert pnames == names and rec.tobytes() == prec.tobytes() and arena.tobytes() == parena.tobytes()
    hs, ha = AF.freq_host(rec, arena, 2.5, split)
    assert AF.tsv_host(hs, ha, names) == R.meth_freq(tsv, 2.5, split)
    if which == "planted" and not clip and not split:
        # the rule is on the printed text: 2.4951171875 is called at 2.5, 2.494140625 is not
        assert list(rec["llr"][0:5]) == [2.5, -2.5, 2.49, 2.12, 2.38] and list(rec["llr"][5:9]) == [-2.12, -2.38, 0.0, -0.0] and np.signbit(rec["llr"][8])
        # one record short: GBX_ERR_ARG with the needs
        nr, nb = np.zeros(1, np.int64), np.zeros(1, np.int64)
        flat, cr, rl, ra = np.ascontiguousarray(sc.reshape(-1)), np.asarray(contig_of_read, np.int32), np.ascontiguousarray(g["ref_len"], np.int32), np.ascontiguousarray(g["ref_arena"], np.uint8)
        r2, a2 = np.zeros(len(rec), AF.RECORD_DTYPE), np.zeros(len(arena), np.uint8)
        rc = AF._lib().gbx_abea_freq_records_host(len(sites), N.ptr(sites), N.ptr(flat), 5, N.ptr(cr), N.ptr(ref_off), N.ptr(rl), N.ptr(ra), lo, hi, len(rec) - 1, N.ptr(r2),
                                                  N.ptr(nr), len(arena), N.ptr(a2), N.ptr(nb))
        assert rc == N.GBX_ERR_ARG and (nr[0], nb[0]) == (len(rec), len(arena)) and not r2.view(np.uint8).any()


# ------------------------------------------------------------------------------------------------ merge
@pytest.mark.parametrize("split", [False, True])
def test_merge(split):
    a_rows, b_rows = K.random_rows(31, 3000, 500), K.random_rows(32, 2500, 500)
    # a site whose first group size differs between the two halves, and one only B's first record fixes
    a_rows += [("chr1", 5, 5, "3.00", 1, "AACGA"), ("chr2", 6, 6, "1.00", 4, "CGCGCGCG")]
    b_rows = [("chr1", 5, 5, "-3.00", 1 if split else 3, "TTCGCGCGT"), ("chr2", 6, 6, "-3.00", 1, "TCGT")] + b_rows
    rows = a_rows + b_rows
    names = sorted({r[0].encode() for r in rows})
    rank = {n: k for k, n in enumerate(names)}

    def dev(rs):
        rec, arena, own = K.to_records(rs)
        rec["contig"] = [rank[own[c]] for c in rec["contig"]]                                 # one rank space for both halves
        return on_device(rec, arena, names, 2.5, split)
    da, db = dev(a_rows), dev(b_rows)
    want = R.table(K.ref_records(rows), 2.5, split)
    m = da.merge(db)
    ms, ma = m.results()
    assert K.table_rows(ms, ma, names) == want and m.text(names) == R.text_of(want)
    whole = dev(rows).results()
    assert ms.tobytes() == whole[0].tobytes() and ma.tobytes() == whole[1].tobytes()
    assert [w for w in want if w[:3] == (b"chr1", 5, 5)][0][6] == b"AACGA" and [w for w in want if w[:3] == (b"chr2", 6, 6)][0][3:] == (1, 1, 0, b"TCGT")
    sa, aa = da.results()
    sb, ab = db.results()
    hs, ha = AF.merge_host(sa, aa, sb, ab)
    assert hs.tobytes() == ms.tobytes() and ha.tobytes() == ma.tobytes()
    # an empty table on either side changes nothing
    empty = dev([])
    assert empty.n_sites == 0
    for x, y, (ws, wa) in ((da, empty, (sa, aa)), (empty, da, (sa, aa)), (empty, empty, (sa[:0], aa[:0]))):
        s, a = x.merge(y).results()
        assert K.table_rows(s, a, names) == K.table_rows(ws, wa, names)
    s, a = AF.merge_host(sa[:0], aa[:0], sb, ab)
    assert K.table_rows(s, a, names) == K.table_rows(sb, ab, names)
    assert len(AF.merge_host(sa[:0], aa[:0], sb[:0], ab[:0])[0]) == 0


# ------------------------------------------------------------------------------------------------ capacities
def test_device_capacities_are_respected():
    import torch
    rows = K.random_rows(41, 2000, 600)
    rec, arena, names = K.to_records(rows)
    full = on_device(rec, arena, names)
    fs, fa = full.results()
    d = AF.DeviceAbeaFreq(device(), 2.5, False, contig_bits=2)
    d.add_records(rec, arena)
    d.count()
    d.size()
    scap, bcap = d.n_sites - 5, int(fs["seq_off"][d.n_sites - 9])
    d.site_cap, d.seq_cap = scap, bcap
    d.sites = torch.full((d.n_sites * 40 + 256,), CANARY, dtype=torch.uint8, device=d.device)
    d.seq_arena = torch.full((d.n_bytes + 256,), CANARY, dtype=torch.uint8, device=d.device)
    off_before, counts_before = d.item_off.cpu().numpy().copy(), d.counts.cpu().numpy().copy()
    d.fill()
    hs, ha = d.sites.cpu().numpy(), d.seq_arena.cpu().numpy()
    assert hs[:scap * 40].tobytes() == fs[:scap].tobytes() and (hs[scap * 40:] == CANARY).all()
    assert ha[:bcap].tobytes() == fa[:bcap].tobytes() and (ha[bcap:] == CANARY).all()
    assert np.array_equal(d.item_off.cpu().numpy(), off_before) and np.array_equal(d.counts.cpu().numpy(), counts_before)
    # the merge's fill
    m = full.merge(full, site_cap=scap, seq_cap=bcap)
    m.sites = torch.full((full.n_sites * 40 + 256,), CANARY, dtype=torch.uint8, device=d.device)
    m.seq_arena = torch.full((full.n_bytes + 256,), CANARY, dtype=torch.uint8, device=d.device)
    m.fill()
    hs, ha = m.sites.cpu().numpy(), m.seq_arena.cpu().numpy()
    assert (hs[scap * 40:] == CANARY).all() and (ha[bcap:] == CANARY).all() and ha[:bcap].tobytes() == fa[:bcap].tobytes()
    twice = hs[:scap * 40].view(AF.FSITE_DTYPE)
    assert np.array_equal(twice["called_sites"], 2 * fs["called_sites"][:scap]) and np.array_equal(twice["group_size"], fs["group_size"][:scap])
    # a wrong item count is flagged and follows no sequence reference
    d2 = AF.DeviceAbeaFreq(device(), 2.5, True, contig_bits=2)
    d2.add_records(rec, arena)
    d2.count()
    true_items = int(d2.counts[0].item())
    d2.counts[0] = true_items - 3
    with pytest.raises(N.GbxError) as e:
        d2.size()
    assert e.value.code == N.GBX_ERR_ARG and d2.flags & AF.ITEMS


def test_host_capacities():
    rows = K.random_rows(43, 500, 100)
    rec, arena, names = K.to_records(rows)
    hs, ha = AF.freq_host(rec, arena)
    for scap, bcap in ((len(hs) - 1, len(ha)), (len(hs), len(ha) - 1), (0, 0)):
        with pytest.raises(N.GbxError) as e:
            AF.freq_host(rec, arena, site_cap=scap, seq_cap=bcap)
        assert e.value.code == N.GBX_ERR_ARG and "%d sites and %d sequence bytes" % (len(hs), len(ha)) in str(e.value)
    s2, a2 = AF.freq_host(rec, arena, site_cap=len(hs), seq_cap=len(ha))
    assert s2.tobytes() == hs.tobytes() and a2.tobytes() == ha.tobytes()


def test_a_sum_above_int_max_is_unsupported():
    rows = [("chr1", 5, 5, "3.00", 2 ** 30, "ACG"), ("chr1", 9, 9, "3.00", 1, "ACG"), ("chr1", 5, 5, "-3.00", 2 ** 30, "ACG"), ("chr1", 5, 5, "3.00", 1, "ACG")]
    rec, arena, names = K.to_records(rows)
    with pytest.raises(N.GbxError) as e:
        AF.freq_host(rec, arena)
    assert e.value.code == N.GBX_ERR_UNSUPPORTED and "INT32_MAX" in str(e.value)
    d = AF.DeviceAbeaFreq(device(), 2.5, False, contig_bits=1)
    d.add_records(rec, arena)
    d.count()
    with pytest.raises(N.GbxError) as e:
        d.size()
    assert e.value.code == N.GBX_ERR_UNSUPPORTED and d.flags == AF.SUM_OVERFLOW
    rec["n_cpg"][2] = 2 ** 30 - 2                                                              # 2^30 + 2^30 - 2 + 1: INT32_MAX itself is inside
    hs, ha = AF.freq_host(rec, arena)
    assert K.table_rows(hs, ha, names) == [(b"chr1", 5, 5, 2 ** 30, 2 ** 31 - 1, 2 ** 30 + 1, b"ACG"), (b"chr1", 9, 9, 1, 1, 1, b"ACG")]
    assert AF.tsv_host(hs, ha, names, with_header=False).startswith(b"chr1\t5\t5\t1073741824\t2147483647\t1073741825\t0.500\tACG\n")


def test_records_device_capacities_are_respected(chained):
    """gbx_abea_freq_records_device FILL with less room than the need: the records and bytes that fit, nothing behind either capacity"""
    import torch
    g, ref_off, sites, scores, planted = chained
    dev = device()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    n = len(sites)
    contig = np.asarray([0, 0, 2, 0, 1], np.int32)
    lo = int(np.sort(sites["start_position"])[40])                                            # a clip, so that the fill compacts
    d_sites, d_scores = t(sites.view(np.uint8).reshape(-1)), t(planted.reshape(-1))
    d_contig, d_roff, d_rlen = t(contig), t(ref_off), t(np.ascontiguousarray(g["ref_len"], np.int32))
    d_ref = t(np.concatenate([np.ascontiguousarray(g["ref_arena"], np.uint8), np.zeros(16, np.uint8)]))
    work = torch.zeros(int(AF._lib().gbx_abea_freq_records_work(n)), dtype=torch.uint8, device=dev)
    off = torch.full((2 * (n + 1) + 8,), -7, dtype=torch.int64, device=dev)
    want_rec, want_arena = AF.records_host(sites, planted, contig, ref_off, g["ref_len"], g["ref_arena"], lo, -1)
    nr, nb = len(want_rec), len(want_arena)
    assert 0 < nr < n

    def run(pass_, rcap, bcap, rec, arena):
        N.check(AF._lib().gbx_abea_freq_records_device(pass_, n, d_sites.data_ptr(), d_scores.data_ptr(), 5, d_contig.data_ptr(), d_roff.data_ptr(), d_rlen.data_ptr(),
                                                       d_ref.data_ptr(), lo, -1, work.data_ptr(), off.data_ptr(), rcap, rec.data_ptr(), bcap, arena.data_ptr(), None))
    for rcap, bcap in ((nr, nb), (nr - 7, int(want_rec["seq_off"][nr - 11])), (0, 0), (nr, 1), (1, nb)):
        rec = torch.full((nr * 40 + 256,), CANARY, dtype=torch.uint8, device=dev)
        arena = torch.full((nb + 256,), CANARY, dtype=torch.uint8, device=dev)
        run(AF.COUNT, 0, 0, rec, arena)
        assert (rec.cpu().numpy() == CANARY).all() and (arena.cpu().numpy() == CANARY).all()   # the count pass writes neither
        run(AF.FILL, rcap, bcap, rec, arena)
        h_off, h_rec, h_arena = off.cpu().numpy(), rec.cpu().numpy(), arena.cpu().numpy()
        assert h_off[n] == nr and h_off[2 * n + 1] == nb and (h_off[2 * (n + 1):] == -7).all()
        assert h_rec[:rcap * 40].tobytes() == want_rec[:rcap].tobytes() and (h_rec[rcap * 40:] == CANARY).all()
        # a record's bytes are written iff they end inside the room; what is not written stays as it was
        ends = want_rec["seq_off"] + want_rec["seq_len"]
        expect = np.full(nb + 256, CANARY, np.uint8)
        for r in np.flatnonzero(ends[:rcap] <= bcap):
            o = int(want_rec["seq_off"][r])
            expect[o:o + int(want_rec["seq_len"][r])] = want_arena[o:o + int(want_rec["seq_len"][r])]
        assert np.array_equal(h_arena, expect)
        if (rcap, bcap) == (nr - 7, int(want_rec["seq_off"][nr - 11])):
            assert h_arena[:bcap].tobytes() == want_arena[:bcap].tobytes() and (h_arena[bcap:] == CANARY).all()


def test_merge_of_a_site_whose_first_records_had_weight_zero():
    """The one documented difference between merge(A, B) and the table of A ++ B, at threshold 0 only: a table holds no site whose
    records all had weight 0, so such records of A do not fix group size 0 and their sequence for B's calls at that key."""
    a_rows = [("chr1", 6, 6, "0.00", 0, "CCC"), ("chr1", 9, 9, "1.00", 1, "ACG")]
    b_rows = [("chr1", 6, 6, "0.50", 3, "CGCGCG")]
    whole = R.table(K.ref_records(a_rows + b_rows), 0.0, False)
    assert whole == [(b"chr1", 6, 6, 0, 3, 3, b"CCC"), (b"chr1", 9, 9, 1, 1, 1, b"ACG")]
    names = [b"chr1"]
    da, db = on_device(*K.to_records(a_rows), thr=0.0), on_device(*K.to_records(b_rows), thr=0.0)
    assert K.table_rows(*da.results(), names) == [(b"chr1", 9, 9, 1, 1, 1, b"ACG")]
    ms, ma = da.merge(db).results()
    assert K.table_rows(ms, ma, names) == [(b"chr1", 6, 6, 3, 3, 3, b"CGCGCG"), (b"chr1", 9, 9, 1, 1, 1, b"ACG")]
    d, want = check_rows(a_rows + b_rows, thr=0.0)                                            # one call over A ++ B is the reference's answer
    assert want == whole


def test_on_a_stream_of_the_callers(chained):
    """every method on a stream other than torch's current one: the same table and text"""
    import torch
    st = torch.cuda.Stream()
    s = st.cuda_stream
    rows = K.edge_rows() + K.random_rows(77, 3000, 500)
    rec, arena, names = K.to_records(rows)
    want = R.table(K.ref_records(rows), 2.5, True)
    d = AF.DeviceAbeaFreq(device(), 2.5, True, contig_bits=AF.bits_for(len(names)))
    cut = int(rec["seq_off"][1000])                                                           # two batches, each with its own arena
    second = rec[1000:].copy()
    second["seq_off"] -= cut
    d.add_records(rec[:1000], arena[:cut])
    d.add_records(second, arena[cut:])
    d.count(s)
    d.size(stream=s)
    d.fill(s)
    sites, seqs = d.results(s)
    assert K.table_rows(sites, seqs, names) == want and d.text(names, stream=s) == R.text_of(want)
    m = d.merge(d, stream=s)
    ms, ma = m.results(s)
    assert np.array_equal(ms["called_sites"], 2 * sites["called_sites"]) and ma.tobytes() == seqs.tobytes()
    g, ref_off, sm, scores, planted = chained
    contigs = [0, 0, 2, 0, 1]
    e = AF.DeviceAbeaFreq(device(), 2.5, False, contig_bits=2)
    e.add_sites(sm, planted.reshape(-1), contigs, ref_off, g["ref_len"], g["ref_arena"], stream=s)
    e.count(s)
    e.size(stream=s)
    e.fill(s)
    rec2, arena2 = AF.records_host(sm, planted, contigs, ref_off, g["ref_len"], g["ref_arena"])
    hs, ha = AF.freq_host(rec2, arena2)
    es, ea = e.results(s)
    assert es.tobytes() == hs.tobytes() and ea.tobytes() == ha.tobytes()
