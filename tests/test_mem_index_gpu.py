"""The HIP index builder on the GPU (gbx_fmi_build_device / _host, gbx_mem_index_build, `mem index`): byte for byte the tables of
the restatement (tests/mem_index_ref.py) where the genome is small, of fmi.build_index otherwise; the doubling rounds of
tests/mem_index_cases.py; canaries behind every output; the host refusals; and the aligner and the driver on an index built this
way against the same on an index from fmi.build_index.  The path is integer: there is no tolerance."""
import ctypes as C
import functools
import os
import subprocess
import threading

import numpy as np
import pytest

from genomicsbench_amd import _native as N
from genomicsbench_amd import fmi as FM
from genomicsbench_amd import mem_align as MA
import mem_align_cases as KA
import mem_index_cases as K
import mem_index_ref as R

pytestmark = pytest.mark.gpu
BIN = os.path.join(os.path.dirname(os.path.abspath(MA.__file__)), "bin", "mem")
CANARY, SLACK = 0xA5, 256
NAMES = sorted(K.SMALL) + sorted(K.LARGE)


@functools.lru_cache(maxsize=None)
def genome(name):
    g = (K.SMALL.get(name) or K.LARGE[name])()
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def expected(name):
    """{sa_compx: dict(ref_seq_len, count, sentinel_index, cp_occ, ms, ls as bytes)}: the restatement's for the small genomes,
    fmi.build_index's on the CPU for the large ones (one build; the samples of sa_compx 3 are every eighth of sa_compx 0's)."""
    g = genome(name)
    if name in K.SMALL:
        return {c: R.build(g, c) for c in (3, 0)}
    idx, smp0 = FM.build_index(g, sa_compx=0)
    out = {}
    for c, smp in ((0, smp0), (3, FM.FmiSa.from_sa(smp0.values()[:idx.ref_seq_len], 3))):
        out[c] = dict(ref_seq_len=idx.ref_seq_len, count=idx.count, sentinel_index=idx.sentinel_index, cp_occ=idx.cp_occ.tobytes(),
                      ms=smp.ms.tobytes(), ls=smp.ls.astype("<u4").tobytes())
    return out


def same(want, idx, smp, what):
    idx, smp = idx.host(), smp.host()
    assert (idx.ref_seq_len, idx.count, idx.sentinel_index) == (want["ref_seq_len"], want["count"], want["sentinel_index"]), what
    assert idx.cp_occ.tobytes() == want["cp_occ"], what
    assert smp.ms.tobytes() == want["ms"] and smp.ls.astype("<u4").tobytes() == want["ls"], what


def check_info(info, want, name):
    assert [info["count%d" % c] for c in range(5)] == want["count"] and info["sentinel_index"] == want["sentinel_index"]
    print(name, "rounds", info["rounds"], "first round slots", info["first_round_slots"])
    if K.ROUNDS[name] is not None:
        assert info["rounds"] == K.ROUNDS[name]
    assert (info["first_round_slots"] == 0) == (info["rounds"] == 0)


@pytest.mark.parametrize("name", NAMES)
def test_build_index_native_on_the_device(name):
    import torch
    g = genome(name)
    for c in (3, 0):
        idx, smp, info = FM.build_index_native(g, "cuda:0", sa_compx=c, info=True)
        assert isinstance(idx.cp_occ, torch.Tensor) and idx.cp_occ.is_cuda and smp.ms.dtype == torch.uint8 and smp.ls.dtype == torch.int32
        same(expected(name)[c], idx, smp, (name, c))
        check_info(info, expected(name)[c], name)
    only = FM.build_index_native(g, "cuda:0")
    assert isinstance(only, FM.FmiIndex) and only.host().cp_occ.tobytes() == expected(name)[3]["cp_occ"]


@pytest.mark.parametrize("name", NAMES)
def test_build_host(name):
    g = genome(name)
    for c in (3, 0):
        idx, smp, info = FM.build_index_native(g, sa_compx=c, info=True)
        assert isinstance(idx.cp_occ, np.ndarray) and idx.cp_occ.dtype == FM.CP_OCC_DTYPE and smp.ms.dtype == np.int8 and smp.ls.dtype == np.uint32
        same(expected(name)[c], idx, smp, (name, c))
        check_info(info, expected(name)[c], name)


def padded(nbytes, torch_dev=None):
    """nbytes and SLACK bytes of canary behind them."""
    if torch_dev is None:
        return np.full(nbytes + SLACK, CANARY, dtype=np.uint8)
    import torch
    return torch.full((nbytes + SLACK,), CANARY, dtype=torch.uint8, device=torch_dev)


@pytest.mark.parametrize("name", ["len1", "len63", "len65", "polyA300", "random1000", "planted20000"])
def test_text_and_canaries(name):
    """The device entry with its text output, and the host entry, into buffers with a canary pattern behind every output."""
    import torch
    L = FM._build_lib()
    g = genome(name)
    dev = torch.device("cuda:0")
    n1 = 2 * len(g) + 1
    ncp = (n1 >> 6) + 1
    dg = torch.from_numpy(np.array(g)).to(dev)
    text_want = np.concatenate([g, 3 - g[::-1]]).astype(np.uint8).tobytes()
    for c in (3, 0):
        want = expected(name)[c]
        n_sa = FM.FmiSa.n_sa_for(n1, c)
        sizes = dict(cp=ncp * 64, ms=n_sa, ls=4 * n_sa, text=2 * len(g), info=64)
        d = {k: padded(v, dev) for k, v in sizes.items()}
        wb = FM.build_workspace_bytes(len(g))
        work = torch.empty(wb, dtype=torch.uint8, device=dev)
        N.check(L.gbx_fmi_build_device(dg.data_ptr(), len(g), c, d["cp"].data_ptr(), d["ms"].data_ptr(), d["ls"].data_ptr(), d["text"].data_ptr(),
                                       d["info"].data_ptr(), work.data_ptr(), wb, torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        h = {k: v.cpu().numpy() for k, v in d.items()}
        for k, v in sizes.items():
            assert (h[k][v:] == CANARY).all(), (name, c, k)
        assert h["cp"][:sizes["cp"]].tobytes() == want["cp_occ"] and h["ms"][:n_sa].tobytes() == want["ms"] and h["ls"][:4 * n_sa].tobytes() == want["ls"]
        assert h["text"][:2 * len(g)].tobytes() == text_want
        words = h["info"][:64].view(np.int64)
        assert list(words[:5]) == want["count"] and words[5] == want["sentinel_index"]
        assert K.ROUNDS[name] is None or words[6] == K.ROUNDS[name]
        # the host entry
        b = {k: padded(sizes[k]) for k in ("cp", "ms", "ls")}
        st, info = FM.FmiIndexStruct(), np.zeros(8, np.int64)
        ga = np.array(g)
        N.check(L.gbx_fmi_build_host(N.ptr(ga), len(g), c, C.addressof(st), N.ptr(b["cp"]), N.ptr(b["ms"]), N.ptr(b["ls"]), N.ptr(info)))
        for k in b:
            assert (b[k][sizes[k]:] == CANARY).all(), (name, c, k)
        assert b["cp"][:sizes["cp"]].tobytes() == want["cp_occ"] and b["ms"][:n_sa].tobytes() == want["ms"] and b["ls"][:4 * n_sa].tobytes() == want["ls"]
        assert (st.ref_seq_len, list(st.count), st.sentinel_index) == (n1, want["count"], want["sentinel_index"]) and st.cp_occ == b["cp"].ctypes.data
        assert np.array_equal(info, words)
        # info may be null
        N.check(L.gbx_fmi_build_host(N.ptr(ga), len(g), c, C.addressof(st), N.ptr(b["cp"]), N.ptr(b["ms"]), N.ptr(b["ls"]), None))


def refusal(rc, code, *words):
    msg = N.lib().gbx_last_error().decode()
    assert rc == code, (rc, msg)
    for w in words:
        assert w in msg, msg
    return msg


def test_host_refusals():
    """None of these reaches the device: the outputs keep their pattern, and nothing of the refused size is allocated."""
    import torch
    L = FM._build_lib()
    ARG, UNS = N.GBX_ERR_ARG, N.GBX_ERR_UNSUPPORTED
    g = np.array(genome("random1000"))
    n1 = 2 * len(g) + 1
    cp, ms, ls = padded(((n1 >> 6) + 1) * 64), padded(n1), padded(4 * n1)
    st = FM.FmiIndexStruct()
    host = lambda genome, l_pac, c: L.gbx_fmi_build_host(N.ptr(genome), l_pac, c, C.addressof(st), N.ptr(cp), N.ptr(ms), N.ptr(ls), None)
    refusal(host(g, 0, 3), ARG, "l_pac = 0")
    refusal(host(g, -5, 3), ARG, "l_pac")
    bad = g.copy(); bad[700] = 4; bad[900] = 9
    refusal(host(bad, len(g), 3), ARG, "base 700", "code 4")
    refusal(host(g, len(g), 1), ARG, "sa_compx = 1")
    refusal(L.gbx_fmi_build_host(None, len(g), 3, C.addressof(st), N.ptr(cp), N.ptr(ms), N.ptr(ls), None), ARG, "null")
    refusal(L.gbx_fmi_build_host(N.ptr(g), len(g), 3, C.addressof(st), None, N.ptr(ms), N.ptr(ls), None), ARG, "null")
    for l_pac in (1 << 31, 1 << 40):                      # the number only: g has 1000 bases
        refusal(host(g, l_pac, 3), UNS, "2^32 - 1")
    assert (cp == CANARY).all() and (ms == CANARY).all() and (ls == CANARY).all()
    # the device entry
    dev = torch.device("cuda:0")
    dg = torch.from_numpy(g).to(dev)
    out = [padded(len(cp) - SLACK, dev), padded(n1, dev), padded(4 * n1, dev), padded(64, dev)]
    wb = FM.build_workspace_bytes(len(g))
    work = torch.empty(wb, dtype=torch.uint8, device=dev)
    devcall = lambda l_pac, c, w, gp=dg.data_ptr(): L.gbx_fmi_build_device(gp, l_pac, c, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), None,
                                                                         out[3].data_ptr(), work.data_ptr(), w, None)
    refusal(devcall(len(g), 3, wb - 1), ARG, "workspace too small", str(wb))
    refusal(devcall(len(g), 3, 0), ARG, "workspace too small")
    refusal(devcall(0, 3, wb), ARG, "l_pac = 0")
    refusal(devcall(len(g), 2, wb), ARG, "sa_compx = 2")
    refusal(devcall(len(g), 3, wb, gp=None), ARG, "null")
    refusal(devcall(1 << 31, 3, wb), UNS, "2^32 - 1")
    assert FM.build_workspace_bytes(1 << 31) == 0
    torch.cuda.synchronize()
    for t in out:
        assert bool((t == CANARY).all())
    # gbx_mem_index_build: the same checks, then the contig table's
    ML = MA.lib()
    h = C.c_void_p()
    co, cn, cno = np.array([0, 400, 1000], np.int64), np.frombuffer(b"ab", np.uint8).copy(), np.array([0, 1, 2], np.int64)
    mem = lambda genome, l_pac, off=co: ML.gbx_mem_index_build(N.ptr(genome), l_pac, 2, N.ptr(off), N.ptr(cn), N.ptr(cno), C.byref(h))
    refusal(mem(bad, len(g)), ARG, "base 700")
    refusal(mem(g, 1 << 31), UNS, "2^32 - 1")
    refusal(mem(g, 0), ARG, "l_pac = 0")
    refusal(mem(g, len(g), np.array([0, 400, 999], np.int64)), ARG, "contig_off")
    assert not h.value
    # and a good call still works afterwards
    N.check(host(g, len(g), 3))
    assert cp[:len(cp) - SLACK].tobytes() == expected("random1000")[3]["cp_occ"]


# ---- the aligner and the driver on an index built on the device
CONTIG_OFF = np.array([0, 9_000, 20_000], dtype=np.int64)
CONTIG_NAMES = ["ctg_one", "ctg_two"]
N_PAIRS = 200


@functools.lru_cache(maxsize=None)
def align_case():
    """20 kbp in two contigs, 200 simulated pairs, and what the aligner makes of them on an index from fmi.build_index."""
    g = KA.genome(8302)[:20_000].copy()
    rs, names, qual = KA.pairs(g, N_PAIRS, 8312)
    ix = MA.MemIndex(g, CONTIG_OFF, CONTIG_NAMES)
    want = MA.MemAligner(ix).run(rs, names, qual, id0=0)
    return g, rs, names, qual, ix.header(), want


def test_mem_index_build_equals_mem_index_create():
    g, rs, names, qual, header, want = align_case()
    ix = MA.MemIndex.build(g, CONTIG_OFF, CONTIG_NAMES)
    assert ix.header() == header and ix.l_pac == len(g)
    got = MA.MemAligner(ix).run(rs, names, qual, id0=0)
    KA.same_output(got, want)
    assert len(got["sam"]) > 100 * N_PAIRS and int((got["recs"]["flag"] & 0x4 == 0).sum()) >= 300       # the reads do align
    ix.close()


def test_driver_index_then_align(tmp_path):
    """`mem index ref.fa` then `mem ref.fa r1.fq r2.fq`, as child processes with a time limit each."""
    g, rs, names, qual, header, want = align_case()
    fa = str(tmp_path / "ref.fa")
    letters = "".join("ACGT"[c] for c in g)
    with open(fa, "w") as f:
        for k, n in enumerate(CONTIG_NAMES):
            seq = letters[int(CONTIG_OFF[k]):int(CONTIG_OFF[k + 1])]
            f.write(">%s\n" % n + "".join(seq[a:a + 70] + "\n" for a in range(0, len(seq), 70)))
    run = lambda *a: subprocess.run(["timeout", "-k", "10", "120", BIN] + list(a), capture_output=True)
    made = run("index", fa)
    assert made.returncode == 0, made.stderr.decode()
    assert "doubling rounds" in made.stderr.decode()
    idx, smp = FM.load_bwa_mem2_index(fa, with_sa=True)
    widx, wsmp = FM.build_index(g, sa_compx=3)
    assert (idx.ref_seq_len, idx.count, idx.sentinel_index) == (widx.ref_seq_len, widx.count, widx.sentinel_index)
    assert idx.cp_occ.tobytes() == widx.cp_occ.tobytes() and smp.sa_compx == 3 and smp.ms.tobytes() == wsmp.ms.tobytes() and smp.ls.tobytes() == wsmp.ls.tobytes()
    saved = str(tmp_path / "saved")
    FM.save_bwa_mem2_index(widx, saved, sa=wsmp)
    MA.save_reference(saved, g, CONTIG_OFF, CONTIG_NAMES)
    for e in (".bwt.2bit.64", ".ann", ".pac", ".0123"):
        assert open(fa + e, "rb").read() == open(saved + e, "rb").read(), e
    lt = KA.letters_of(rs)
    fq = []
    for e in (0, 1):
        path = str(tmp_path / ("r%d.fq" % (e + 1)))
        with open(path, "w") as f:
            f.write(KA.fastq(names[e::2], lt[e::2], qual, rs.read_off[e::2], suffix="/%d" % (e + 1)))
        fq.append(path)
    got = run(fa, *fq)
    assert got.returncode == 0, got.stderr.decode()
    assert got.stdout == header + want["sam"]


def test_two_host_threads():
    """Two host threads build two different genomes at once through gbx_fmi_build_host."""
    names = ["planted20000", "tandem2000"]
    for n in names:
        expected(n)
    out, err = {}, []

    def work(n):
        try:
            out[n] = [FM.build_index_native(genome(n), sa_compx=3, info=True) for _ in range(2)]
        except Exception as e:                            # noqa: BLE001
            err.append(e)
    th = [threading.Thread(target=work, args=(n,)) for n in names]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not err, err
    for n in names:
        for idx, smp, info in out[n]:
            same(expected(n)[3], idx, smp, n)
            assert info["rounds"] == K.ROUNDS[n]
