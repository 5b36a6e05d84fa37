"""Index construction without a GPU: the restatement (tests/mem_index_ref.py) against fmi.build_index, which pins the two
witnesses the GPU tests compare the HIP builder with; `mem index --parse-only` against mem_align.save_reference and against the
restatement; and csrc/drivers/ref_files.h under ASan + UBSan in a program of its own (tests/sanitize_ref)."""
import functools
import os
import subprocess

import numpy as np
import pytest

from genomicsbench_amd import fmi as FM
from genomicsbench_amd import mem_align as MA
import mem_index_cases as K
import mem_index_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "genomicsbench_amd", "bin", "mem")
SAN = os.path.join(ROOT, "tests", "sanitize_ref")
EXT = (".ann", ".amb", ".pac", ".0123")


def same_as_build_index(want, idx, smp):
    assert want["ref_seq_len"] == idx.ref_seq_len and want["count"] == idx.count and want["sentinel_index"] == idx.sentinel_index
    assert want["cp_occ"] == idx.cp_occ.tobytes()
    assert want["ms"] == smp.ms.tobytes() and want["ls"] == smp.ls.astype("<u4").tobytes()


@pytest.mark.parametrize("name", sorted(K.SMALL) + ["planted20000"])
def test_restatement_equals_build_index(name):
    g = (K.SMALL.get(name) or K.LARGE[name])()
    for sa_compx in (3, 0):
        same_as_build_index(R.build(g, sa_compx), *FM.build_index(g, sa_compx=sa_compx))


def test_lrand48_restatement():
    """srand48(11), eight draws (glibc's lrand48: checked against libc when the restatement was written)."""
    r = R.Rand48(11)
    got = [r.next() for _ in range(8)]
    import ctypes
    libc = ctypes.CDLL(None)
    libc.lrand48.restype = ctypes.c_long
    libc.srand48(11)
    assert got == [libc.lrand48() for _ in range(8)]


def fasta_text(contigs, wrap=60, eol="\n"):
    out = []
    for head, seq in contigs:
        out.append(">" + head + eol)
        out += [seq[k:k + wrap] + eol for k in range(0, len(seq), wrap)]
    return "".join(out).encode()


def parse_only(path, *opts):
    return subprocess.run([BIN, "index", "--parse-only"] + list(opts) + [path], capture_output=True, timeout=60)


def files(prefix):
    return {e: open(prefix + e, "rb").read() for e in EXT}


def test_parse_only_equals_save_reference(tmp_path):
    g = K.rand(1_003, 7801)
    off = np.array([0, 401, 1_003], dtype=np.int64)
    names = ["chrA", "chrB.2"]
    letters = "".join("ACGT"[c] for c in g)
    letters = letters[:100] + letters[100:250].lower() + letters[250:900] + letters[900:].lower()
    fa = str(tmp_path / "ref.fa")
    with open(fa, "wb") as f:
        f.write(fasta_text([(names[0], letters[:401]), (names[1], letters[401:])], wrap=60, eol="\r\n"))
    r = parse_only(fa)
    assert r.returncode == 0, r.stderr.decode()
    want = str(tmp_path / "want")
    MA.save_reference(want, g, off, names)
    got = files(fa)
    for e in (".ann", ".pac", ".0123"):
        assert got[e] == open(want + e, "rb").read(), e
    assert got[".amb"] == b"1003 2 0\n"
    head = r.stdout.decode().splitlines()
    assert head[0].startswith("l_pac=1003 contigs=2 holes=0 text_checksum=") and head[1] == "contig 0 chrA 0 401 0" and head[2] == "contig 1 chrB.2 401 602 0"
    # -p names the prefix
    r = parse_only(fa, "-p", str(tmp_path / "other"))
    assert r.returncode == 0 and files(str(tmp_path / "other")) == got


def test_parse_only_holes_equal_the_restatement(tmp_path):
    """N and R runs at a contig's start, in its interior, at its end and across a line break; comments; a second contig that starts
    with the character the first ended in (a new hole: holes do not cross contigs)."""
    body = K.rand(400, 7802)
    s = "".join("ACGT"[c] for c in body)
    c1 = "NNN" + s[:50] + "RR" + s[50:53] + "NNNNNNNN" + s[53:200] + "nN" + s[200:230] + "NN"          # wrap 60: the 8 N straddle a line break
    c2 = "NNNN" + s[230:300] + "RRRRRYK" + s[300:]
    data = fasta_text([("one first contig, with a comment", c1), ("two\tcomment two", c2)], wrap=60)
    fa = str(tmp_path / "holes.fa")
    with open(fa, "wb") as f:
        f.write(data)
    r = parse_only(fa)
    assert r.returncode == 0, r.stderr.decode()
    want, codes = R.reference_files(data)
    got = files(fa)
    for e in EXT:
        assert got[e] == want[e], e
    amb = got[".amb"].decode().splitlines()
    assert amb[0] == "%d 2 10" % len(codes) and amb[1] == "0 3 N" and amb[3] == "58 8 N" and amb[4:6] == ["213 1 n", "214 1 N"]
    ann = got[".ann"].decode().splitlines()
    assert ann[1] == "0 one first contig, with a comment" and ann[2].endswith(" 6") and ann[3] == "0 two comment two" and ann[4].endswith(" 4")
    # the replaced bases are draws of lrand48 after srand48(11), in file order
    rng = R.Rand48(11)
    holes = [l.split() for l in amb[1:]]
    for off, ln, _ in holes:
        for k in range(int(off), int(off) + int(ln)):
            assert codes[k] == rng.next() & 3
    # mem's own .ann reader takes the comments and the non-zero n_ambs (its --parse-only prints the reference when .ann exists)
    fq = str(tmp_path / "r.fq")
    with open(fq, "w") as f:
        f.write("@r0\nACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIII\n")
    m = subprocess.run([BIN, "--parse-only", fa, fq], capture_output=True, timeout=60)
    assert m.returncode == 0, m.stderr.decode()
    lines = m.stdout.decode().splitlines()
    assert r.stdout.decode().split("text_checksum=")[1][:16] in "".join(lines) and "contig 0 one 0 %d" % len(c1) in lines and \
        "contig 1 two %d %d" % (len(c1), len(c2)) in lines


BAD = {
    "empty": (b"", "empty"),
    "blank": (b"\n\n", "empty"),
    "no_header": (b"ACGT\n>x\nACGT\n", "before any header"),
    "no_bases": (b">x\nACGT\n>y\n>z\nAC\n", "no bases"),
    "no_bases_last": (b">x\nACGT\n>y\n", "no bases"),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_parse_only_errors(tmp_path, name):
    data, word = BAD[name]
    fa = str(tmp_path / "bad.fa")
    with open(fa, "wb") as f:
        f.write(data)
    r = parse_only(fa)
    err = r.stderr.decode()
    assert r.returncode == 1 and word in err and len(err.strip().splitlines()) == 1, err


def test_index_refuses_other_options_and_missing_files(tmp_path):
    fa = str(tmp_path / "x.fa")
    with open(fa, "wb") as f:
        f.write(b">x\nACGT\n")
    for opt in (["-a", "bwtsw"], ["-b", "1000"], ["-6"]):
        r = subprocess.run([BIN, "index"] + opt + [fa], capture_output=True, timeout=60)
        assert r.returncode == 1 and ("option %s is not supported" % opt[0]) in r.stderr.decode()
    r = parse_only(str(tmp_path / "absent.fa"))
    assert r.returncode == 1 and "cannot read" in r.stderr.decode()


def test_the_limit_is_the_builders():
    """ref_files.h names the same limit gbx_fmi_build_* has: 2 l_pac + 1 <= 2^32 - 1."""
    h = open(os.path.join(ROOT, "genomicsbench_amd", "csrc", "drivers", "ref_files.h")).read()
    assert "MAX_L_PAC = 2147483647" in h and 2 * 2147483647 + 1 == 2 ** 32 - 1
    assert FM.build_workspace_bytes(2147483647) > 0 and FM.build_workspace_bytes(2147483648) == 0 and FM.build_workspace_bytes(0) == 0
    # the workspace formula stays below 48 bytes per text symbol
    for l_pac in (1 << 20, 1 << 26, 2147483647):
        assert 38 * 2 * l_pac < FM.build_workspace_bytes(l_pac) < 40 * 2 * l_pac + (1 << 16)


@functools.lru_cache(maxsize=None)
def san_exe():
    r = subprocess.run(["make", "-C", SAN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return os.path.join(SAN, "_build", "ref_main")


def test_ref_files_under_asan_ubsan(tmp_path):
    """The stand-alone program over good files, the bad ones, a file cut mid-line and a file with a 1 MB header line: clean, and
    the same summary as the driver's."""
    s = "".join("ACGT"[c] for c in K.rand(500, 7803))
    good = {
        "plain.fa": fasta_text([("a", s[:300]), ("b c", s[300:])]),
        "crlf_holes.fa": fasta_text([("a x", "NN" + s[:100] + "RRN" + s[100:200] + "N"), ("b", "N" + s[200:])], wrap=17, eol="\r\n"),
        "cut.fa": fasta_text([("a", s[:130])])[:-9],                     # ends inside a sequence line, no newline
        "cut_header.fa": b">a\nACGT\n>b partial comm",                   # ends inside a header: contig b has no bases
        "long_header.fa": b">n " + b"x" * (1 << 20) + b"\nACGTN\n",
        "long_name.fa": b">" + b"y" * (1 << 20) + b"\nACGT\n",
        "one_base.fa": b">a\nA",
        "odd_bytes.fa": b">a\nAC\x00GT \tac\xff*\n",
    }
    paths = []
    for name, data in list(good.items()) + [(k + ".fa", v[0]) for k, v in BAD.items()]:
        p = str(tmp_path / name)
        with open(p, "wb") as f:
            f.write(data)
        paths.append(p)
    out = tmp_path / "out"
    out.mkdir()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([san_exe(), str(out)] + paths, capture_output=True, text=True, timeout=300, env=env)
    bad = [w for w in ("AddressSanitizer", "runtime error:", "LeakSanitizer") if w in r.stderr or w in r.stdout]
    assert r.returncode == 0 and not bad, r.stdout[-1500:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(paths)
    status = dict(zip([os.path.basename(p) for p in paths], lines))
    for k in BAD:
        assert status[k + ".fa"].startswith("error: ") and BAD[k][1] in status[k + ".fa"]
    assert status["cut_header.fa"].startswith("error: ") and status["long_name.fa"].startswith("error: ")
    assert status["cut.fa"].startswith("ok l_pac=122 ") and status["one_base.fa"].startswith("ok l_pac=1 ")
    assert status["long_header.fa"].startswith("ok l_pac=5 contigs=1 holes=1 ") and status["odd_bytes.fa"].startswith("ok l_pac=7 contigs=1 holes=1 ")
    # the driver says the same of the files that parse, and the restatement writes the same files
    for k, name in enumerate(os.path.basename(p) for p in paths):
        if not status[name].startswith("ok"):
            continue
        d = parse_only(str(tmp_path / name))
        assert d.returncode == 0 and d.stdout.decode().splitlines()[0] == status[name][3:]
        want, _ = R.reference_files(open(str(tmp_path / name), "rb").read())
        for e in EXT:
            assert open(str(out / str(k)) + e, "rb").read() == want[e] == open(str(tmp_path / name) + e, "rb").read(), (name, e)
