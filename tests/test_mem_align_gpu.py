"""The aligner (gbx_mem_aligner_*, genomicsbench_amd/mem_align.py) and the mem driver on the GPU.  The expected output is always the
existing composition of the stage classes (tests/mem_align_cases.py: mem_sam.pipeline and its parts, generous capacities, none
overflowed), never the aligner itself, and the comparison is byte for byte: the path is integer and text, so there is no
tolerance."""
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
from genomicsbench_amd import mem_chain as MC
from genomicsbench_amd import mem_cigar as MG
from genomicsbench_amd import mem_pair as MP
from genomicsbench_amd import mem_sam as SM
import mem_align_cases as K
import mem_sam_ref as R

pytestmark = pytest.mark.gpu
N_PAIRS, ID0 = 60, 500
BIN = os.path.join(os.path.dirname(os.path.abspath(MA.__file__)), "bin", "mem")


@functools.lru_cache(maxsize=None)
def genome():
    return K.genome()


@functools.lru_cache(maxsize=None)
def index():
    return MA.MemIndex(genome(), K.CONTIG_OFF, K.CONTIG_NAMES)


@functools.lru_cache(maxsize=None)
def case1():
    """The 60 pairs and what the composition makes of them with id0 = 500."""
    rs, names, qual = K.pairs(genome(), N_PAIRS, 8311)
    return rs, names, qual, K.compose_paired(genome(), rs, names, qual, ID0)


def test_paired_equals_the_composition():
    rs, names, qual, want = case1()
    al = MA.MemAligner(index())
    got = al.run(rs, names, qual, id0=ID0)
    K.same_output(got, want)
    text = MC.text_of(genome())
    assert R.validate(got["sam"], text, K.CONTIG_NAMES, K.CONTIG_OFF, got["recs"]) == len(got["recs"])
    assert al.header() == SM.header(K.CONTIG_NAMES, K.CONTIG_OFF, len(genome())).encode()
    # the input exercises the path
    flags = got["recs"]["flag"]
    assert int(((flags & 0x800) != 0).sum()) >= 5
    assert b"H" in b"".join(l.split(b"\t")[5] for l in got["sam"].split(b"\n")[:-1])
    assert int(((flags & 0x2) != 0).sum()) >= 80
    assert int((want["rescue_stats"]["n_kept"] > 0).sum()) >= 1
    st = got["stats"]
    assert st["runs"] == 1 and st["counts"]["n_recs"] == len(got["recs"]) and st["counts"]["n_text"] == len(got["sam"])
    assert st["counts"]["n_xregs"] > st["counts"]["n_regs"] > 0 and st["bytes_up"] > len(rs.enc) and st["bytes_down"] >= len(got["sam"])


def test_single_end_equals_the_composition():
    g = genome()
    rs, names, qual, _ = K.mixed(g, 80, 8411)
    want = K.compose_single(g, rs, names, qual, 7)
    al = MA.MemAligner(index(), MA.default_params(mode=0))
    got = al.run(rs, names, qual, id0=7)
    K.same_output(got, want, pes=False)
    assert (got["pes"]["failed"] == 1).all()
    assert R.validate(got["sam"], MC.text_of(g), K.CONTIG_NAMES, K.CONTIG_OFF, got["recs"]) == len(got["recs"])
    for r in (3, 5):                                     # all N; 12 bases, below min_seed_len
        a, b = got["rec_off"][r], got["rec_off"][r + 1]
        assert b - a == 1 and got["recs"]["flag"][a] == 0x4 and got["recs"]["rid"][a] == -1
    assert int((got["recs"]["flag"] & 0x4 == 0).sum()) >= 60
    # without qualities QUAL prints *
    plain = al.run(rs, names, None, id0=7)
    assert plain["sam"] == K.compose_single(g, rs, names, None, 7)["sam"] and all(l.split(b"\t")[10] == b"*" for l in plain["sam"].split(b"\n")[:-1])


def tiny_caps():
    p = MA.default_params()
    z = MG.lib().gbx_mem_cigar_record_z_bytes(C.byref(p.cigar), 101, 301)         # the room of one record
    kw = {n: 64 for n in MA.CAP_FIELDS if n not in ("z_bytes",)}
    return MA.make_caps(z_bytes=z, **kw)


def test_overflow_and_rerun():
    rs, names, qual, want = case1()
    al = MA.MemAligner(index(), first_caps=tiny_caps())
    got = al.run(rs, names, qual, id0=ID0)
    K.same_output(got, want)
    st = got["stats"]
    print("reruns", st["reruns"], "from", [MA.STAGES[k] for k in st["rerun_stage"]], "caps", st["caps"], "counts", st["counts"])
    assert st["reruns"] >= 1
    c, n = st["caps"], st["counts"]
    for cap, cnt in zip(MA.CAP_FIELDS[1:], MA.COUNT_FIELDS[1:16]):
        if cap != "z_bytes":
            assert c[cap] >= n[cnt] >= 0, (cap, cnt)
    assert n["n_z_miss"] == 0 and n["slot_worst"] == 0
    assert st["reruns"] - st["slot_reruns"] <= len(MA.CAP_FIELDS)
    assert st["rerun_stage"] == sorted(st["rerun_stage"])          # what lies before an overflow is never recomputed


def test_state_does_not_leak():
    g = genome()
    a = K.pairs(g, 20, 8511)
    b = case1()
    want_a = K.compose_paired(g, a[0], a[1], a[2], 0)
    al = MA.MemAligner(index())
    got_a = al.run(*a, id0=0)
    got_b = al.run(b[0], b[1], b[2], id0=20)
    again = al.run(*a, id0=0)
    K.same_output(got_a, want_a)
    K.same_output(got_b, K.compose_paired(g, b[0], b[1], b[2], 20))
    K.same_output(again, want_a)
    assert again["sam"] == got_a["sam"] and again["recs"].tobytes() == got_a["recs"].tobytes()
    assert again["stats"]["runs"] == 3
    nb, na = got_b["stats"]["counts"], got_a["stats"]["counts"]
    assert nb["n_text"] > 2 * na["n_text"] and nb["n_pos"] > 2 * na["n_pos"] and got_b["stats"]["bytes_up"] > 2 * got_a["stats"]["bytes_up"]    # B needs larger buffers


PES = [(0, 0, 1, 0., 0.), (120, 480, 0, 300., 28.), (0, 0, 1, 0., 0.), (1, 900, 0, 310.5, 110.25)]


def test_given_estimate():
    rs, names, qual, _ = case1()
    want = K.compose_variant(genome(), rs, names, qual, ID0, pes=PES)
    p = MA.set_pes(MA.default_params(), PES)
    al = MA.MemAligner(index(), p)
    N.profile_begin()
    got = al.run(rs, names, qual, id0=ID0)
    prof = N.profile_end(256)
    K.same_output(got, want)
    assert got["pes"].tobytes() == MP.pestat_records(PES).tobytes()
    assert "mem_pestat" not in prof and any(k.startswith("mem_rescue") for k in prof) and "mem_align_gather" in prof
    # and the stage is there when no estimate is given
    N.profile_begin()
    MA.MemAligner(index()).run(rs, names, qual, id0=ID0)
    assert "mem_pestat" in N.profile_end(256)


def test_no_rescue_and_no_pairing():
    rs, names, qual, base = case1()
    g = genome()
    p = MA.default_params()
    p.no_rescue = 1
    got = MA.MemAligner(index(), p).run(rs, names, qual, id0=ID0)
    K.same_output(got, K.compose_variant(g, rs, names, qual, ID0, no_rescue=True))
    assert got["sam"] != base["sam"] and got["stats"]["counts"]["n_xregs"] == 0
    p = MA.default_params()
    p.pair.no_pairing = 1
    got = MA.MemAligner(index(), p).run(rs, names, qual, id0=ID0)
    K.same_output(got, K.compose_variant(g, rs, names, qual, ID0, no_pairing=True))
    assert got["sam"] != base["sam"]


def run_pair(entry, rsc, pes_arg):
    """One of the two paired entries behind the rescue stage `rsc`, into fresh outputs -> the DeviceMemPair that holds them."""
    import torch
    pe = MP.DeviceMemPair(rsc, MP.make_params())
    sd, b = rsc.seeds, rsc.batch
    N.check(entry(C.byref(pe.params), pe.n_pairs, pe.pair_id0, rsc.regs.data_ptr(), rsc.reg_off.data_ptr(), rsc.counts.data_ptr(), rsc.reg_cap,
                  rsc.sel_seeds.data_ptr(), rsc.sel_res.data_ptr(), rsc.sel_cap, sd.seeds.data_ptr(), sd.cap, sd.l_rep.data_ptr(),
                  b.l_pac, b.n_contigs, b.contig_off.data_ptr(), pes_arg, pe.pes.data_ptr(), pe.pairs.data_ptr(), pe.pregs.data_ptr(),
                  pe.psel_seeds.data_ptr(), pe.psel_res.data_ptr(), pe.psel_cap, pe.count.data_ptr(), pe.work.data_ptr(), pe.work_bytes, None))
    torch.cuda.synchronize()
    return pe.results()


def same_pair(a, b):
    for k in ("pes", "pairs", "pregs", "psel_seeds", "psel_res"):
        assert np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes(), k
    assert a["n_psel"] == b["n_psel"]


def test_pair_device_pes():
    import torch
    want = case1()[3]
    rg, rsc, pe = want["stages"][:3]
    L = MA.lib()
    host = rsc.pes_host(None)
    assert (host["failed"] == 0).any()
    by_host = run_pair(MP.lib().gbx_mem_pair_device, rsc, N.ptr(host))
    same_pair(by_host, pe.results())
    same_pair(run_pair(L.gbx_mem_pair_device_pes, rsc, rsc.pes.data_ptr()), by_host)
    same_pair(run_pair(L.gbx_mem_pair_device_pes, rsc, None), run_pair(MP.lib().gbx_mem_pair_device, rsc, None))
    # a record pes_check refuses of a host pointer is taken as failed on the device
    bad = host.copy()
    d = int(np.flatnonzero(bad["failed"] == 0)[0])
    bad["std"][d] = 0.
    with pytest.raises(N.GbxError):
        run_pair(MP.lib().gbx_mem_pair_device, rsc, N.ptr(bad))
    failed = bad.copy()
    failed["failed"][d] = 1
    d_bad = torch.from_numpy(bad.view(np.uint8).copy()).cuda()
    same_pair(run_pair(L.gbx_mem_pair_device_pes, rsc, d_bad.data_ptr()), run_pair(MP.lib().gbx_mem_pair_device, rsc, N.ptr(failed)))


def refused(al, code, **kw):
    rs, names, qual = K.pairs(genome(), 4, 8611)
    nm, no = SM.arena(names)
    a = dict(n_reads=rs.n_reads, enc=rs.enc, read_off=rs.read_off.copy(), read_len=rs.read_len.copy(), qual=qual, name_arena=nm, name_off=no, id0=0)
    a.update(kw)
    before = al.stats()["runs"]
    with pytest.raises(N.GbxError) as e:
        al.run_arrays(**a)
    assert e.value.code == code, str(e.value)
    assert al.stats()["runs"] == before
    return str(e.value)


def test_host_checks():
    rs, names, qual = K.pairs(genome(), 4, 8611)
    al = MA.MemAligner(index())
    al.run(rs, names, qual)
    assert al.stats()["runs"] == 1
    ARG, UNS = N.GBX_ERR_ARG, N.GBX_ERR_UNSUPPORTED
    assert "odd" in refused(al, ARG, n_reads=7)
    off = rs.read_off.copy(); off[3] = off[2] - 1
    assert "read 3" in refused(al, ARG, read_off=off)
    off = rs.read_off.copy(); off[7] = len(rs.enc) - 100
    assert "read 7" in refused(al, ARG, read_off=off)
    ln = rs.read_len.copy(); ln[2] = 0
    assert "read 2" in refused(al, ARG, read_len=ln)
    no = SM.arena(names)[1]; no[4] = no[3] - 1
    assert "read 3" in refused(al, ARG, name_off=no)
    refused(al, ARG, id0=-1)
    refused(al, ARG, id0=(1 << 23) - 3)
    long_enc = np.zeros(8 * 1025, np.uint8)
    long = dict(enc=long_enc, read_off=np.arange(8, dtype=np.int64) * 1025, read_len=np.full(8, 1025, np.int32), qual=None)
    assert "read 0" in refused(al, UNS, **long)
    se = MA.MemAligner(index(), MA.default_params(mode=0))
    assert se.run_arrays(7, rs.enc, rs.read_off, rs.read_len, qual, *SM.arena(names[:7]), id0=(1 << 24) - 7)["stats"]["runs"] == 1     # odd counts and 1025 bases are fine there
    huge = dict(n_reads=1, enc=np.zeros(8193, np.uint8), read_off=np.zeros(1, np.int64), read_len=np.full(1, 8193, np.int32), qual=None,
                name_arena=np.frombuffer(b"x", np.uint8).copy(), name_off=np.array([0, 1], np.int64))
    before = se.stats()["runs"]
    with pytest.raises(N.GbxError) as e:
        se.run_arrays(**huge)
    assert e.value.code == UNS and se.stats()["runs"] == before
    # a caller's estimate that pes_check refuses, and copies that disagree: no aligner is made
    with pytest.raises(N.GbxError) as e:
        MA.MemAligner(index(), MA.set_pes(MA.default_params(), [(1, 500, 0, 300., 0.)] * 4))
    assert e.value.code == ARG
    p = MA.default_params()
    p.rescue.T = 31
    with pytest.raises(N.GbxError) as e:
        MA.MemAligner(index(), p)
    assert e.value.code == ARG and "T" in str(e.value)
    # the aligner still works after the refusals
    K.same_output(al.run(rs, names, qual), K.compose_paired(genome(), rs, names, qual, 0))


def test_four_host_threads():
    rs, names, qual, want = case1()
    ix = index()
    out, err = [None] * 4, []

    def work(k):
        try:
            out[k] = MA.MemAligner(ix).run(rs, names, qual, id0=ID0)
        except Exception as e:                            # noqa: BLE001
            err.append(e)
    th = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not err, err
    for o in out:
        K.same_output(o, want)


def test_driver_end_to_end(tmp_path):
    rs, names, qual, _ = case1()
    g = genome()
    prefix = str(tmp_path / "ref")
    idx, smp = FM.build_index(g, sa_compx=3)
    FM.save_bwa_mem2_index(idx, prefix, sa=smp)
    MA.save_reference(prefix, g, K.CONTIG_OFF, K.CONTIG_NAMES)
    letters = K.letters_of(rs)
    fq = []
    for e in (0, 1):
        path = str(tmp_path / ("r%d.fq" % (e + 1)))
        with open(path, "w") as f:
            f.write(K.fastq(names[e::2], letters[e::2], qual, rs.read_off[e::2], suffix="/%d" % (e + 1)))
        fq.append(path)
    run = lambda *a: subprocess.run([BIN] + list(a), capture_output=True, timeout=120)
    parsed = run("--parse-only", "-K", "4000", prefix, *fq)
    assert parsed.returncode == 0, parsed.stderr.decode()
    batches = [dict(kv.split("=") for kv in l.split()[2:]) for l in parsed.stdout.decode().splitlines() if l.startswith("batch ")]
    assert len(batches) >= 3 and sum(int(b["reads"]) for b in batches) == rs.n_reads
    al = MA.MemAligner(index())
    want, at = al.header(), 0
    for b in batches:
        n = int(b["reads"])
        assert int(b["id0"]) == at // 2
        sub = rs.take(at, at + n)
        a0 = int(rs.read_off[at])
        want += al.run(sub, names[at:at + n], qual[a0:a0 + len(sub.enc)], id0=at // 2)["sam"]
        at += n
    got = run("-K", "4000", "-t", "2", prefix, *fq)
    assert got.returncode == 0, got.stderr.decode()
    assert got.stdout == want
    out = str(tmp_path / "out.sam")
    one = run("-K", "4000", "-t", "1", "-o", out, prefix, *fq)
    assert one.returncode == 0 and one.stdout == b"", one.stderr.decode()
    with open(out, "rb") as f:
        assert f.read() == want
