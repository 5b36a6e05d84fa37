"""CPU-side checks for the minimizer seeding stage: the restatement (tests/mm_ref.py) on the cross-check vectors of its rules, the
device's machine compiled for the host in pieces against it, the exported symbols, the parameter and host-entry refusals (all
before a device is touched) and the mmseed driver's command line."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from genomicsbench_amd import _native as N
from genomicsbench_amd import mm_seed as MS
import mm_cases as K
import mm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MMSEED = os.path.join(ROOT, "genomicsbench_amd", "bin", "mmseed")


def test_hash_vectors():
    assert R.hash64(0x1234567, 2 ** 30 - 1) == 0x5a86716
    assert R.hash64(0, 2 ** 30 - 1) == 0x3ff06f15
    assert R.hash64(2 ** 56 - 1, 2 ** 56 - 1) == 0xfa4d157df516b7


def test_sketch_vectors():
    assert [R.unpack(m) for m in R.sketch(K.SEVENTEEN, 3, 3)] == [(23, 3, 4, 1), (26, 3, 6, 1), (33, 3, 7, 0), (15, 3, 10, 0), (12, 3, 12, 1),
                                                                  (5, 3, 15, 0), (5, 3, 16, 1)]
    s = "ACGGGGTTTACCCCCCAGTNACGTTTGCAAAAC"
    m = R.sketch(s, 4, 5, 7)
    assert [R.unpack(v)[2] for v in m] == [7, 8, 12, 14, 27, 28, 29, 32] and all(y >> 32 == 7 for _, y in m)
    assert [R.unpack(v) for v in R.sketch(s, 4, 5, 7, True)] == [(781, 7, 26, 0)]
    st = {}
    assert len(R.sketch("ATATATGCGCATTAATCGAT", 2, 4, stats=st)) == 11 and st["symmetric"] == 6
    assert R.sketch("AT" * 40, 2, 4) == []                                   # every k-mer is its own reverse complement
    assert len(R.sketch("ACGTAC", 10, 5)) == 1                               # shorter than w + k - 1: the flush gives one


def test_sketch_magnitudes():
    rng = random.Random(5)
    s = K.rand_seq(rng, 10000)
    for (w, k, hpc), want in (((10, 15, 0), 1872), ((10, 19, 1), 1338), ((19, 19, 0), 992), ((1, 28, 0), 9973)):
        n = len(R.sketch(s, w, k, 0, bool(hpc)))
        assert abs(n - want) <= 0.05 * want, (w, k, hpc, n)


def test_homopolymer_under_hpc():
    s = K.rand_seq(random.Random(6), 60) + b"A" * 300 + K.rand_seq(random.Random(7), 60)
    m = R.sketch(s, 10, 19, 0, True)
    assert m and all(x & 0xff < 256 for x, _ in m)
    for x, y in m:                                                           # no minimizer's span reaches into the run
        end, span = (y & 0xffffffff) >> 1, x & 0xff
        assert end < 60 or end - span + 1 >= 360


@pytest.mark.parametrize("w,k,hpc", K.SKETCH_PARAMS)
def test_emission_order_is_ascending_y(w, k, hpc):
    """What the index's stable sort by key relies on: a sequence's minimizers come out in ascending, distinct y."""
    _, y, off = K.sketch_expected(w, k, hpc)
    for s in range(len(off) - 1):
        assert (np.diff(y[off[s]:off[s + 1]].astype(np.int64)) > 0).all()


def _twin():
    L = C.CDLL(os.path.join(ROOT, "genomicsbench_amd", "libgbx_mm_cpu.so"))
    L.gbx_mm_cpu_sketch.restype = C.c_int64
    L.gbx_mm_cpu_sketch.argtypes = [C.c_char_p, C.c_int64, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64]
    return L


def _twin_sketch(L, s, w, k, rid, hpc, chunk):
    ox, oy = np.zeros(len(s) + 1, np.uint64), np.zeros(len(s) + 1, np.uint64)
    n = L.gbx_mm_cpu_sketch(bytes(s), len(s), w, k, rid, hpc, chunk, N.ptr(ox), N.ptr(oy), len(ox))
    assert n <= len(s)                                                       # a base ends one minimizer at most
    return list(zip(ox[:n].tolist(), oy[:n].tolist()))


def test_machine_in_pieces_equals_the_restatement():
    """The device's machine (mm_machine.h, compiled for the host) taken in warm-started pieces of any size gives the full run:
    odd k in pieces of 1 .. 256 bases, even k as a whole."""
    L = _twin()
    rng = random.Random(11)
    for t in range(600):
        s = K.rand_seq(rng, rng.randint(0, 400), rng.choice(["ACGT", "AC", "ACGTN", "AT", "ACGTNNNN", "AAAC"]))
        w, k, hpc = rng.randint(1, 20), rng.randint(1, 12), rng.random() < .5
        chunk = rng.choice([1, 2, 3, 7, 16, 50, 256]) if k & 1 else 0
        assert _twin_sketch(L, s, w, k, 3, int(hpc), chunk) == R.sketch(s, w, k, 3, hpc), (s, w, k, hpc, chunk)


@pytest.mark.parametrize("w,k,hpc", K.SKETCH_PARAMS)
def test_machine_on_the_sketch_cases(w, k, hpc):
    L = _twin()
    x, y, off = K.sketch_expected(w, k, hpc)
    for rid, s in enumerate(K.sketch_batch(w, k, hpc)):
        got = _twin_sketch(L, s, w, k, rid, hpc, K.CHUNK if k & 1 else 0)
        assert got == list(zip(x[off[rid]:off[rid + 1]].tolist(), y[off[rid]:off[rid + 1]].tolist())), rid


def test_mid_occ_rule():
    assert R.mid_occ_of([1] * 9999 + [7], 2e-4) == 2                          # rank (uint32)(0.9998 * 10000) = 9997
    assert R.mid_occ_of([1, 2, 3, 50], 2e-4) == 51
    assert R.mid_occ_of([1, 2, 3, 50], 0.5) == 4
    assert R.mid_occ_of([1, 2, 3, 50], 0.0) == R.INT32_MAX and R.mid_occ_of([], 0.5) == R.INT32_MAX
    assert R.mid_occ_of([1, 2, 3, 50], 2e-4, explicit=3) == 3


def test_symbols_exported():
    L = N.lib()
    for name in ("default_params", "check_params", "sketch_workspace_bytes", "sketch_device", "sketch_host", "index_bytes",
                 "index_workspace_bytes", "index_build_device", "index_build_host", "index_stats", "seed_workspace_bytes", "seed_device",
                 "seed_host"):
        assert hasattr(L, "gbx_mm_" + name), name


def test_default_params():
    p = MS.make_params()
    assert (p.k, p.w, p.is_hpc, p.mid_occ, p.max_gap, p.bw) == (15, 10, 0, 0, 5000, 500)
    assert p.mid_occ_frac == np.float32(2e-4)
    MS.check_params(p)


@pytest.mark.parametrize("kw,word", [(dict(k=0), "k ="), (dict(k=29), "k ="), (dict(w=0), "w ="), (dict(w=256), "w ="),
                                     (dict(max_gap=-1), "max_gap"), (dict(bw=-1), "bw"), (dict(mid_occ=-1), "mid_occ"),
                                     (dict(mid_occ_frac=1.0), "mid_occ_frac"), (dict(mid_occ_frac=float("nan")), "mid_occ_frac")])
def test_check_params_refuses(kw, word):
    with pytest.raises(N.GbxError) as e:
        MS.check_params(MS.make_params(**kw))
    assert e.value.code == N.GBX_ERR_ARG and word in str(e.value)


def _sketch_host_rc(p, n, seq, off, mx=True):
    buf = np.zeros(16, np.uint64)
    moff, cnt = np.zeros(8, np.int64), C.c_int64(0)
    return MS.lib().gbx_mm_sketch_host(C.byref(p), n, N.ptr(seq), N.ptr(off), 1, N.ptr(buf) if mx else None, N.ptr(buf), 16, N.ptr(moff), C.byref(cnt))


def test_host_entries_refuse_before_a_device():
    """Null pointers, offsets that decrease and over-long sequences are named without a device (none exists on a CPU-only box, and an
    error other than these would say so)."""
    L, p = MS.lib(), MS.make_params()
    seq = np.frombuffer(b"ACGTACGTACGTACGTACGTACGT", np.uint8).copy()
    i64 = lambda *v: np.array(v, np.int64)
    err = lambda: L.gbx_last_error().decode()
    assert _sketch_host_rc(p, 2, seq, None) == N.GBX_ERR_ARG and "null" in err()
    assert _sketch_host_rc(p, 2, None, i64(0, 10, 24)) == N.GBX_ERR_ARG and "null" in err()
    assert _sketch_host_rc(p, 2, seq, i64(0, 10, 24), mx=False) == N.GBX_ERR_ARG and "null" in err()
    assert _sketch_host_rc(p, 2, seq, i64(1, 10, 24)) == N.GBX_ERR_ARG and "seq_off[0]" in err()
    assert _sketch_host_rc(p, 3, seq, i64(0, 12, 10, 24)) == N.GBX_ERR_ARG and "not monotone at sequence 1" in err()
    assert _sketch_host_rc(p, 2, seq, i64(0, 10, 10 + 2 ** 31)) == N.GBX_ERR_UNSUPPORTED and "sequence 1" in err()
    assert _sketch_host_rc(MS.make_params(k=29), 2, seq, i64(0, 10, 24)) == N.GBX_ERR_ARG and "k = 29" in err()
    # index
    keys, koff, vals, st = np.zeros(32, np.uint64), np.zeros(33, np.int64), np.zeros(32, np.uint64), MS.MmIndexInfo()
    build = lambda n, s, o, k_=keys, st_=C.byref(st): L.gbx_mm_index_build_host(C.byref(p), n, N.ptr(s), N.ptr(o), N.ptr(k_), N.ptr(koff), 32, N.ptr(vals), 32, st_)
    assert build(2, seq, None) == N.GBX_ERR_ARG and "null" in err()
    assert build(2, seq, i64(0, 10, 24), k_=None) == N.GBX_ERR_ARG and "null" in err()
    assert build(2, seq, i64(0, 10, 24), st_=None) == N.GBX_ERR_ARG and "null" in err()
    assert build(3, seq, i64(0, 12, 10, 24)) == N.GBX_ERR_ARG and "not monotone at sequence 1" in err()
    assert build(3, seq, i64(0, 4, 4 + 2 ** 31, 5 + 2 ** 31)) == N.GBX_ERR_UNSUPPORTED and "sequence 1" in err()
    # seeding
    ax, off, hdr = np.zeros(64, np.uint64), np.zeros(8, np.int64), np.zeros(4, N.CHAIN_CALL_DTYPE)
    rep, cnt = np.zeros(4, np.int32), np.zeros(2, np.int64)
    koff[:] = 0

    def seed(n, s, o, koff_=koff, n_keys=0, off_=off, n_ref=1):
        return L.gbx_mm_seed_host(C.byref(p), N.ptr(keys), N.ptr(koff_), n_keys, N.ptr(vals), 10, n_ref, 1000, n, N.ptr(s), N.ptr(o), None, None, 0, None,
                                  N.ptr(ax), N.ptr(ax), 64, N.ptr(off_), N.ptr(hdr), N.ptr(rep), N.ptr(rep), N.ptr(cnt))
    assert seed(2, seq, None) == N.GBX_ERR_ARG and "null" in err()
    assert seed(2, seq, i64(0, 10, 24), off_=None) == N.GBX_ERR_ARG and "null" in err()
    assert seed(2, seq, i64(0, 10, 24), koff_=None) == N.GBX_ERR_ARG and "null" in err()
    assert seed(3, seq, i64(0, 12, 10, 24)) == N.GBX_ERR_ARG and "not monotone at read 1" in err()
    assert seed(2, seq, i64(0, 10, 10 + 2 ** 31)) == N.GBX_ERR_UNSUPPORTED and "read 1" in err()
    assert seed(2, seq, i64(0, 10, 24), koff_=i64(0, 5, 3), n_keys=2) == N.GBX_ERR_ARG and "key_off is not monotone at key 1" in err()
    assert seed(2, seq, i64(0, 10, 24), n_ref=2 ** 31) == N.GBX_ERR_UNSUPPORTED
    assert seed(0, seq, i64(0)) == N.GBX_OK and cnt[0] == 0 and cnt[1] == 0


def test_device_entries_refuse_bad_arguments():
    L, p = MS.lib(), MS.make_params()
    assert L.gbx_mm_sketch_device(C.byref(p), 1, None, None, 10, 1, None, None, 0, None, None, None, 0, None) == N.GBX_ERR_ARG
    assert L.gbx_mm_index_build_device(C.byref(p), 1, None, None, 10, None, 10, None, 0, None) == N.GBX_ERR_ARG
    assert L.gbx_mm_seed_device(C.byref(p), None, 1, 1, 1, MS.MAX_READS + 1, None, None, 0, None, None, 0, None, None, None, 0, None, None, None,
                                None, None, None, 0, None) == N.GBX_ERR_UNSUPPORTED
    assert L.gbx_mm_index_bytes(1000) >= 256 + 3 * 8000 and L.gbx_mm_seed_workspace_bytes(C.byref(p), 4, 1000, 1000, 4000) > 0
    assert L.gbx_mm_seed_workspace_bytes(C.byref(MS.make_params(w=0)), 4, 1000, 1000, 4000) == 0


def test_mmseed_command_line(tmp_path):
    run = lambda *a: subprocess.run([MMSEED] + list(a), capture_output=True, text=True, timeout=60)
    r = run("--help")
    assert r.returncode == 0 and r.stdout.startswith("usage: mmseed") and "--mid-occ" in r.stdout
    for args, word in ((("-k",), "-k takes an integer"), (("-k", "x", "a", "b"), "-k takes an integer"), (("-q", "a", "b"), "unknown option -q"),
                       (("a",), "a reference and a read file"), (("-k", "29", "a", "b"), "k = 29"), (("-w", "0", "a", "b"), "w = 0"),
                       (("-g", "-1", "a", "b"), "max_gap"), (("-f", "z", "a", "b"), "-f takes a number")):
        r = run(*args)
        assert r.returncode == 1 and word in r.stderr, (args, r.stderr)
    fa = tmp_path / "ref.fa"
    fa.write_text(">r\nACGT\n")
    r = run(str(fa), str(tmp_path / "absent.fq"))
    assert r.returncode == 1 and "fail to open" in r.stderr
