"""CPU tests of kmer-cnt (no GPU): the numpy restatement (tests/kmer_ref.py) against the reference's printed numbers, the
Python reader against the driver's ingest, the driver's config handling and the C-ABI's exported symbols."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

from genomicsbench_amd import kmer as K
import kmer_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BIN = os.path.join(ROOT, "genomicsbench_amd", "bin", "kmer-cnt")
LIB = os.path.join(ROOT, "genomicsbench_amd", "libgbx.so")
RUNS = json.load(open(os.path.join(GOLDEN, "kmer_reference.json")))["runs"]


def golden_reads(names, min_read=5000):
    return K.read_fasta([os.path.join(GOLDEN, n) for n in names], min_read)


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    """The gzipped golden inputs decompressed (bin/kmer-cnt reads plain text): name without .gz -> path."""
    d = tmp_path_factory.mktemp("kmer_plain")
    out = {}
    for n in ("kmer_a.fasta.gz", "kmer_b.fastq.gz"):
        out[n[:-3]] = str(d / n[:-3])
        with gzip.open(os.path.join(GOLDEN, n), "rb") as f, open(out[n[:-3]], "wb") as g:
            g.write(f.read())
    return out


@pytest.mark.parametrize("run", RUNS, ids=lambda r: "%s-k%d" % ("+".join(r["reads"]), r["k"]))
def test_ref_equals_reference_numbers(run):
    st = R.count_ref(golden_reads(run["reads"], run["min_read"]), run["k"])[0]
    assert (st["n_distinct"], st["n_ge16"]) == (run["total_kmers"], run["hash_size"])


def test_goldens_cover_the_edge_cases(plain):
    recs = K.parse_records(os.path.join(GOLDEN, "kmer_a.fasta.gz"))
    assert recs == K.parse_records(plain["kmer_a.fasta"])
    lens = {len(s) for _, s in recs}
    assert {5000, 5001} <= lens
    text = b"".join(s for _, s in recs)
    assert b"N" in text and any(c in text for c in b"RYKMBDHVU") and any(c in text for c in b"acgt")
    assert b"A" * 500 in text
    assert any(r["hash_size"] > 0 for r in RUNS)
    assert max(len(l) for l in open(plain["kmer_a.fasta"], "rb").read().split(b"\n")) <= 81   # wrapped
    rs = golden_reads(["kmer_a.fasta.gz"])
    assert 5001 in rs.read_len.tolist() and 5000 not in rs.read_len.tolist()       # strict '>'


def test_encode_spills_invalid_characters_to_the_chunk_end():
    seq = b"A" * 40 + b"N" + b"C" * 30
    c = K.encode(seq)
    assert c[:40].tolist() == [0] * 40
    assert c[40:64].tolist() == [3] * 24                      # the N and the rest of its 32-base chunk
    assert c[64:].tolist() == [1] * 7
    assert K.encode(b"acgtACGT").tolist() == [0, 1, 2, 3, 0, 1, 2, 3]


def test_ref_last_window_not_counted():
    rs = K.KmerReadSet.from_codes([[0, 1, 2, 3, 0], [1, 1], [2, 2, 2]])
    st, hist, km, cn = R.count_ref(rs, 3, n_hist=8, min_freq=1)
    assert st["n_positions"] == 2
    # ACG (6) / revcomp CGT (27) -> 6; CGT (27) / ACG (6) -> 6: one canonical k-mer counted twice
    assert km.tolist() == [6] and cn.tolist() == [2] and hist.tolist() == [0, 0, 1, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("threads", [1, 3])
def test_read_fasta_equals_driver_parse(plain, threads):
    names = ["kmer_a.fasta.gz", "kmer_b.fastq.gz"]
    out = subprocess.run([BIN, "--reads", ",".join(plain[n[:-3]] for n in names), "--config",
                          os.path.join(GOLDEN, "kmer_k15.cfg"), "--parse-only", "--threads", str(threads)],
                         capture_output=True, text=True, check=True).stdout
    got = json.loads(out.strip().splitlines()[-1])
    rs = golden_reads(names)
    assert (got["reads"], got["bases"], got["fnv1a"]) == (rs.n_reads, rs.n_bases, rs.checksum())


def test_driver_min_read_and_min_ovlp(plain):
    fa = plain["kmer_a.fasta"]
    cfg = os.path.join(GOLDEN, "kmer_k15.cfg")
    for extra, m in ((["--min-ovlp", "1000"], 1000), (["--min-read", "6000"], 6000)):
        out = subprocess.run([BIN, "--reads", fa, "--config", cfg, "--parse-only"] + extra, capture_output=True, text=True, check=True).stdout
        got = json.loads(out.strip().splitlines()[-1])
        rs = K.read_fasta(fa, m)
        assert (got["reads"], got["fnv1a"]) == (rs.n_reads, rs.checksum())


def run_driver(args):
    return subprocess.run([BIN] + args, capture_output=True, text=True)


def test_config_include_and_refusals(plain, tmp_path):
    fa = plain["kmer_a.fasta"]
    sub = tmp_path / "sub"
    sub.mkdir()
    (sub / "base.cfg").write_text("# shared\nkmer_size = 13\nuse_minimizers=0\n")
    (tmp_path / "top.cfg").write_text("%include sub/base.cfg\nassemble_kmer_sample=1\n")
    r = run_driver(["--reads", fa, "--config", str(tmp_path / "top.cfg"), "--parse-only", "--debug"])
    assert r.returncode == 0 and "Running with k-mer size: 13" in r.stderr
    (tmp_path / "mini.cfg").write_text("%include sub/base.cfg\nuse_minimizers=1\n")
    r = run_driver(["--reads", fa, "--config", str(tmp_path / "mini.cfg"), "--parse-only"])
    assert r.returncode != 0 and "minimizer" in r.stderr
    (tmp_path / "nok.cfg").write_text("use_minimizers=0\n")
    r = run_driver(["--reads", fa, "--config", str(tmp_path / "nok.cfg"), "--parse-only"])
    assert r.returncode != 0 and "kmer_size" in r.stderr
    r = run_driver(["--reads", fa, "--config", str(tmp_path / "nok.cfg"), "--kmer", "11", "--parse-only", "--debug"])
    assert r.returncode == 0 and "Running with k-mer size: 11" in r.stderr
    r = run_driver(["--reads", fa, "--config", str(tmp_path / "nok.cfg"), "--kmer", "18", "--parse-only"])
    assert r.returncode != 0
    (tmp_path / "bad.cfg").write_text("kmer_size 15\n")
    assert run_driver(["--reads", fa, "--config", str(tmp_path / "bad.cfg"), "--parse-only"]).returncode != 0
    assert run_driver(["--reads", fa, "--config", str(tmp_path / "missing.cfg"), "--parse-only"]).returncode != 0


def test_driver_refuses_duplicate_ids_and_gzip(plain):
    fa = plain["kmer_a.fasta"]
    r = run_driver(["--reads", fa + "," + fa, "--config", os.path.join(GOLDEN, "kmer_k15.cfg"), "--parse-only"])
    assert r.returncode != 0 and "duplicated IDs" in r.stderr
    r = run_driver(["--reads", os.path.join(GOLDEN, "kmer_a.fasta.gz"), "--config", os.path.join(GOLDEN, "kmer_k15.cfg"), "--parse-only"])
    assert r.returncode != 0 and "gzip" in r.stderr


def test_kmer_symbols_exported():
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout.split()
    for s in ("gbx_kmer_count_host", "gbx_kmer_count_device", "gbx_kmer_workspace_bytes"):
        assert s in syms
    from genomicsbench_amd import _native as N
    L = N.lib()
    assert L.gbx_kmer_workspace_bytes(15, 10, 256) >= 4 << 30
    assert L.gbx_kmer_workspace_bytes(17, 10, 256) < (4 << 30) + (1 << 20)      # one slice of 2^30 counters
    assert L.gbx_kmer_workspace_bytes(18, 10, 256) == 0


def test_host_entry_argument_checks():
    """Refused before any device is touched: bad k, bad n_hist, a read outside enc."""
    from genomicsbench_amd import _native as N
    rs = K.KmerReadSet.from_codes([np.zeros(20, dtype=np.uint8)])
    for kw in (dict(k=0), dict(k=18), dict(k=5, n_hist=1), dict(k=5, n_hist=5000)):
        with pytest.raises(N.GbxError) as e:
            K.count_host(rs, **kw)
        assert e.value.code == N.GBX_ERR_ARG
    bad = K.KmerReadSet(rs.enc, np.array([5], dtype=np.int64), np.array([20], dtype=np.int32))
    with pytest.raises(N.GbxError) as e:
        K.count_host(bad, 5)
    assert e.value.code == N.GBX_ERR_ARG
