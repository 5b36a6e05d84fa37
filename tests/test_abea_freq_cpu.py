"""meth-freq without a GPU: the Python restatement of freq.c against the compiled reference's recorded outputs, the library's
TSV parser against the restatement's, the rules header against the C library in a stand-alone program under ASan + UBSan,
the driver's --parse-only, and what the entries refuse before they touch a device."""
import json
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "abea_freq_reference.json")
SAN = os.path.join(ROOT, "tests", "sanitize_freq")
DRIVER = os.path.join(ROOT, "genomicsbench_amd", "bin", "meth-freq")


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def golden_cases():
    """(name, input bytes, threshold, split, header kind, the reference's output bytes)"""
    g = golden()
    out = []
    for name, o in sorted(g["options"].items()):
        opts = o["opts"]
        thr = float(opts[opts.index("-c") + 1]) if "-c" in opts else 2.5
        out.append((name, g["inputs"]["v%d_k%d" % (o["version"], o["kind"])].encode(), thr, "-s" in opts, o["kind"], g["outputs"][name].encode()))
    return out


def fnv1a(data, h=1469598103934665603):
    for b in bytes(data):
        h = ((h ^ b) * 1099511628211) & (2 ** 64 - 1)
    return h


# ------------------------------------------------------------------------------------------------ the restatement
def test_golden_is_the_edge_batch():
    g = golden()
    assert set(g["outputs"]) >= {"default", "split", "c0", "c5", "strand", "motifs"}
    assert g["inputs"]["v1_k1"].encode() == K.to_text(K.edge_rows(), 1, 1) and g["inputs"]["v2_k1"].encode() == K.to_text(K.edge_rows(), 2, 1)
    assert os.path.getsize(GOLDEN) < 128 * 1024


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c[0])
def test_restatement_equals_golden(case):
    name, text, thr, split, kind, want = case
    assert R.meth_freq(text, thr, split) == want
    assert want.startswith(R.OUT_HEADERS[kind])


def test_golden_holds_the_verified_answers():
    d = golden()["outputs"]["default"]
    assert "chr1\t100\t110\t2\t5\t2\t0.400\tAACGTTACGTA\n" in d                      # first-seen group size and sequence
    assert d.index("chr10\t") < d.index("chr2\t")                                    # strcmp order
    for f in ("\t16\t1\t0.062\t", "\t16\t3\t0.188\t", "\t2000\t9\t0.004\t", "\t2000\t5\t0.003\t", "\t2000\t7\t0.004\t", "\t2000\t1999\t1.000\t"):
        assert f in d
    assert "chr4\t50\t" not in golden()["outputs"]["c0"] and "chr4\t60\t60\t0\t3\t2\t" in golden()["outputs"]["c0"]
    assert "chr3\t1\t1\t1\t2\t1\t0.500\t" in d                                        # NaN kept, unmethylated


# ------------------------------------------------------------------------------------------------ the parser
def _same_parse(text):
    version, kind, want = R.parse(text)
    rec, arena, names, got_kind = AF.parse_tsv(text)
    assert got_kind == kind and names == sorted({r[0] for r in want}) and len(rec) == len(want)
    a = arena.tobytes()
    for c, (chrom, start, end, llr, n, seq) in zip(rec, want):
        assert names[c["contig"]] == chrom and (c["start"], c["end"], c["n_cpg"]) == (start, end, n)
        assert np.float64(c["llr"]).tobytes() == np.float64(llr).tobytes() or (np.isnan(c["llr"]) and np.isnan(llr))
        assert a[c["seq_off"]:c["seq_off"] + c["seq_len"]] == seq
    assert int(rec["seq_len"].sum()) == len(a) and not rec["pad_"].any()
    return rec, arena, names


def test_parser_equals_restatement_on_the_four_headers():
    for version in (1, 2):
        for kind in (1, 2):
            _same_parse(K.to_text(K.edge_rows(), version, kind))
    _same_parse(K.to_text(K.random_rows(5, 3000, 400), 1, 1))
    _same_parse(K.HEAD[(1, 1)].encode())                                              # a header alone: no records


def test_parser_reads_fields_as_the_c_library_does():
    head = K.HEAD[(1, 1)]
    rows = ["chrA\t 12\t+13x\tr\t1e1\t0\t0\t1\t 2 \tACGCG\n",                        # atoi skips blanks and stops at the first non-digit
            "chrA\t\t7\t8\tr\t-.5e+1\t0\t0\t1\t1\tCG\t\n",                           # strtok folds empty fields and a trailing tab
            "chrB\t0\t0\tr\tinfinity\t0\t0\t1\t3\tCGCGCG",                            # no newline at the end of the file
            ]
    rec, arena, names = _same_parse((head + "".join(rows)).encode())
    assert list(rec["start"]) == [12, 7, 0] and list(rec["end"]) == [13, 8, 0] and list(rec["llr"][:2]) == [10.0, -5.0] and np.isinf(rec["llr"][2])


@pytest.mark.parametrize("text,line", [
    (b"", 0),
    (b"chromosome\tstart\n", 0),
    (K.HEAD[(1, 1)].encode()[:-1], 0),                                                # the header without its newline
    ((K.HEAD[(1, 1)] + "chr1\t5\t6\tr\t3.0\t0\t0\t1\t1\n").encode(), 2),             # a column short
    ((K.HEAD[(2, 1)] + "chr1\t5\t6\tr\t3.0\t0\t0\t1\t1\tACG\n").encode(), 2),        # no strand under the strand header
    ((K.HEAD[(1, 1)] + "chr1\t5\t6\tr\t3.0\t0\t0\t1\t1\tACG\nchr1\t5\t6\tr\t3.0\t0\t0\t1\t1\tACG\textra\n").encode(), 3),
    ((K.HEAD[(1, 1)] + "chr1\t-5\t6\tr\t3.0\t0\t0\t1\t1\tACG\n").encode(), 2),
    ((K.HEAD[(1, 1)] + "chr1\t5\t-6\tr\t3.0\t0\t0\t1\t1\tACG\n").encode(), 2),
    ((K.HEAD[(1, 1)] + "chr1\t5\t6\tr\t3.0\t0\t0\t1\t-1\tACG\n").encode(), 2),
    ((K.HEAD[(1, 1)] + "chr1\t5\t6\tr\t3.0\t0\t0\t1\t1\tACG\n\n").encode(), 3),      # an empty line
])
def test_parser_refuses_what_the_reference_refuses(text, line):
    with pytest.raises(R.RefExit) as want:
        R.parse(text)
    with pytest.raises(N.GbxError) as got:
        AF.parse_tsv(text)
    assert got.value.code == N.GBX_ERR_ARG and got.value.message == want.value.message and got.value.bad_line == line == want.value.line


def test_parser_refuses_a_contig_name_with_a_colon():
    with pytest.raises(N.GbxError) as e:
        AF.parse_tsv((K.HEAD[(1, 1)] + "chr1\t5\t6\tr\t3.0\t0\t0\t1\t1\tACG\nHLA:A\t5\t6\tr\t3.0\t0\t0\t1\t1\tACG\n").encode())
    assert e.value.code == N.GBX_ERR_UNSUPPORTED and e.value.bad_line == 3


def test_parser_capacities():
    text = K.to_text(K.edge_rows())
    rec, arena, names, kind = AF.parse_tsv(text)
    buf = np.frombuffer(text, np.uint8)
    counts, k, bad = np.zeros(4, np.int64), np.zeros(1, np.int32), np.zeros(1, np.int64)
    r2, a2, n2 = np.zeros(len(rec), AF.RECORD_DTYPE), np.zeros(len(arena), np.uint8), np.zeros(sum(len(n) + 1 for n in names), np.uint8)
    for short in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
        rc = AF._lib().gbx_abea_freq_parse_host(N.ptr(buf), len(buf), len(r2) - short[0], N.ptr(r2), len(a2) - short[1], N.ptr(a2), len(n2) - short[2], N.ptr(n2),
                                                N.ptr(counts), N.ptr(k), N.ptr(bad))
        assert rc == N.GBX_ERR_ARG and bad[0] == -1 and list(counts) == [len(rec), len(arena), len(names), len(n2)]
    assert AF._lib().gbx_abea_freq_parse_host(N.ptr(buf), len(buf), len(r2), N.ptr(r2), len(a2), N.ptr(a2), len(n2), N.ptr(n2), N.ptr(counts), N.ptr(k), N.ptr(bad)) == 0
    assert r2.tobytes() == rec.tobytes() and a2.tobytes() == arena.tobytes() and n2.tobytes() == b"".join(n + b"\0" for n in names)


# ------------------------------------------------------------------------------------------------ the rules header
def test_rules_under_asan_ubsan():
    """csrc/abea_freq_rules.h built for the host in a stand-alone program under ASan + UBSan: "%.3lf" for every m <= c <= 2048, the
    two-decimal rule for every k / 1024 with |k| <= 16384 and a million seeded float pairs, "%d", the CG step on exact buffers."""
    r = subprocess.run(["make", "-C", SAN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([os.path.join(SAN, "_build", "freq_rules_main")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    words = r.stdout.split()
    assert words[0] == "ok" and int(words[2]) == sum(c + 1 for c in range(1, 2049)) and int(words[4]) >= 2 * 16384 + 1 + 1000000


def test_restatement_of_the_two_decimal_rule():
    """the verified answers of the issue, through printf and strtod themselves"""
    assert R.llr_as_read(2.4951171875) == 2.5 and R.llr_as_read(-2.4951171875) == -2.5 and R.llr_as_read(2.494140625) == 2.49
    assert R.llr_as_read(2.125) == 2.12 and R.llr_as_read(2.375) == 2.38


# ------------------------------------------------------------------------------------------------ the driver
def test_driver_parse_only_on_the_golden_inputs(tmp_path):
    for key, text in sorted(golden()["inputs"].items()):
        rec, arena, names, kind = AF.parse_tsv(text.encode())
        src = tmp_path / (key + ".tsv")
        src.write_bytes(text.encode())
        want = "records %d contigs %d sequence_bytes %d header_kind %d checksum %016x\n" % (
            len(rec), len(names), len(arena), kind, fnv1a(b"".join(n + b"\0" for n in names), fnv1a(arena.tobytes(), fnv1a(rec.tobytes()))))
        r = subprocess.run([DRIVER, "--parse-only", "-i", str(src)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stdout == want, r.stderr
        r = subprocess.run([DRIVER, "--parse-only", "-s", "-c", "1.5"], input=text, capture_output=True, text=True, timeout=60)      # stdin is the default
        assert r.returncode == 0 and r.stdout == want and "Scanning the input from stdin" in r.stderr


def test_driver_exits_as_the_reference_does(tmp_path):
    bad = K.HEAD[(1, 1)] + "chr1\t5\t6\tr\t3.0\t0\t0\t1\t1\tACG\textra\n"
    r = subprocess.run([DRIVER], input=bad, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == "" and R.MORE_COLUMNS % 2 in r.stderr
    r = subprocess.run([DRIVER], input="not a header\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == "" and "Incorrect header: not a header\n" in r.stderr
    r = subprocess.run([DRIVER, "-x"], input="", capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Unrecognized option: -x" in r.stderr and "Usage:" in r.stderr
    r = subprocess.run([DRIVER, "-i", str(tmp_path / "missing.tsv")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "missing.tsv" in r.stderr


# ------------------------------------------------------------------------------------------------ the C-ABI
def test_symbols_exported_and_struct_sizes():
    L = AF._lib()
    for name in ("gbx_abea_freq_work", "gbx_abea_freq_device", "gbx_abea_freq_host", "gbx_abea_freq_records_work", "gbx_abea_freq_records_device",
                 "gbx_abea_freq_records_host", "gbx_abea_freq_merge_device", "gbx_abea_freq_merge_host", "gbx_abea_freq_tsv_work", "gbx_abea_freq_tsv_device",
                 "gbx_abea_freq_tsv_host", "gbx_abea_freq_parse_host"):
        assert hasattr(L, name), name
    assert AF.RECORD_DTYPE.itemsize == 40 and AF.FSITE_DTYPE.itemsize == 40
    assert AF.RECORD_DTYPE.fields["llr"][1] == 16 and AF.RECORD_DTYPE.fields["seq_off"][1] == 24 and AF.FSITE_DTYPE.fields["seq_off"][1] == 24
    w0, w1 = L.gbx_abea_freq_work(1000, 0), L.gbx_abea_freq_work(1000, 5000)
    assert 0 < w0 < w1 and w1 % 256 == 0 and w1 >= 5000 * (32 + 24 + 16 + 8 + 8 + 16)
    assert L.gbx_abea_freq_work(-1, 0) == 0 and L.gbx_abea_freq_tsv_work(-1) == 0 and L.gbx_abea_freq_records_work(-1) == 0
    assert L.gbx_abea_freq_tsv_work(10) > 0 and L.gbx_abea_freq_records_work(10) > 0


def test_argument_errors_come_first():
    """refused on the arguments alone: these pass without a device"""
    L = AF._lib()
    rec, arena, names = K.to_records(K.edge_rows())
    one, cnt = np.zeros(64, np.int64), np.zeros(8, np.int64)
    ns, nb = np.zeros(1, np.int64), np.zeros(1, np.int64)
    p = N.ptr
    host = lambda r, a=arena, n=None: L.gbx_abea_freq_host(len(r) if n is None else n, p(r), p(a), a.size, 2.5, 0, 0, None, p(ns), 0, None, p(nb))
    assert host(rec, n=-1) == N.GBX_ERR_ARG
    assert L.gbx_abea_freq_host(len(rec), p(rec), p(arena), arena.size, 2.5, 0, 0, None, None, 0, None, p(nb)) == N.GBX_ERR_ARG
    assert L.gbx_abea_freq_host(len(rec), None, p(arena), arena.size, 2.5, 0, 0, None, p(ns), 0, None, p(nb)) == N.GBX_ERR_ARG
    for field, value, word in (("start", -1, "record 3"), ("n_cpg", -2, "record 3"), ("contig", -1, "record 3"), ("seq_off", 1 << 40, "record 3"), ("seq_len", -1, "record 3")):
        bad = rec.copy()
        bad[field][3] = value
        assert host(bad) == N.GBX_ERR_ARG and word in L.gbx_last_error().decode()
    assert host(rec[:0]) == 0 and ns[0] == 0                                           # nothing in, nothing out: no device needed
    # device entries: pass, bits, null pointers
    dev = lambda pass_, pos_bits=31, contig_bits=8, work=p(one): L.gbx_abea_freq_device(pass_, 4, p(one), p(one), 2.5, 0, pos_bits, contig_bits, 4, work, p(one),
                                                                                        p(cnt), 0, None, 0, None, None)
    for args in ((0,), (8,), (AF.COUNT | AF.REDUCE,), (AF.REDUCE, 0), (AF.REDUCE, 32), (AF.REDUCE, 31, 0), (AF.REDUCE, 31, 8, None)):
        assert dev(*args) == N.GBX_ERR_ARG
    assert L.gbx_abea_freq_merge_device(AF.COUNT, 0, None, None, 0, None, None, 31, 8, p(one), p(cnt), 0, None, 0, None, None) == N.GBX_ERR_ARG
    assert L.gbx_abea_freq_tsv_device(AF.COUNT, 1, p(one), p(one), 1, p(one), p(one), 3, 1, p(one), p(one), 0, None, None) == N.GBX_ERR_ARG     # header kind
    assert L.gbx_abea_freq_records_device(AF.REDUCE, 1, p(one), p(one), 1, p(one), p(one), p(one), p(one), -1, -1, p(one), p(one), 0, None, 0, None, None) == N.GBX_ERR_ARG
    # tables
    site = np.zeros(2, AF.FSITE_DTYPE)
    site["called_sites"] = 1
    site["seq_len"][1] = 5                                                               # outside an empty arena
    assert L.gbx_abea_freq_merge_host(2, p(site), None, 0, 0, None, None, 0, 0, None, p(ns), 0, None, p(nb)) == N.GBX_ERR_ARG
    assert "site 1 of the first table" in L.gbx_last_error().decode()
    site["seq_len"][1] = -1
    site["contig"][1] = 1
    nm = (N.C.c_char_p * 1)(b"chr1")
    assert L.gbx_abea_freq_tsv_host(2, p(site), None, 0, 1, nm, AF.CPGS, 1, 0, None, p(ns)) == N.GBX_ERR_ARG and "site 1" in L.gbx_last_error().decode()
    assert L.gbx_abea_freq_tsv_host(2, p(site), None, 0, 1, nm, 0, 1, 0, None, p(ns)) == N.GBX_ERR_ARG
    # sites and scores
    ms = np.zeros(2, AF.SITE_DTYPE)
    ms["read"][1] = 7
    sc, cr, ro, rl, ra = np.zeros(4, np.float32), np.zeros(1, np.int32), np.zeros(1, np.int64), np.full(1, 8, np.int32), np.zeros(8, np.uint8)
    assert L.gbx_abea_freq_records_host(2, p(ms), p(sc), 1, p(cr), p(ro), p(rl), p(ra), -1, -1, 0, None, p(ns), 0, None, p(nb)) == N.GBX_ERR_ARG
    assert "site 1 names read 7" in L.gbx_last_error().decode()


def test_without_a_device_the_host_entries_say_so():
    if N.device_count() > 0:
        pytest.skip("a device is present: the GPU tests cover the entries")
    rec, arena, names = K.to_records(K.edge_rows())
    with pytest.raises(N.GbxError) as e:
        AF.freq_host(rec, arena)
    assert e.value.code == N.GBX_ERR_NO_DEVICE
