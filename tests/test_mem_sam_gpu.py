"""SAM records on the GPU (gbx_mem_sam_device / gbx_mem_sam_host), byte-exact against the restated rules of tests/mem_sam_ref.py
on the records, the offsets, the counts, the md bytes and the text, and every line through the independent validator.  No
tolerance: the stage is integer and text."""
import ctypes as C
import threading

import numpy as np
import pytest

from genomicsbench_amd import _native as N
from genomicsbench_amd import fmi as FM
from genomicsbench_amd import mem_chain as MC
from genomicsbench_amd import mem_cigar as MG
from genomicsbench_amd import mem_pair as MP
from genomicsbench_amd import mem_sam as SM
from genomicsbench_amd.mem_pipeline import Stages
import mem_cigar_cases as KG
import mem_rescue_cases as KR
import mem_sam_cases as K
import mem_sam_ref as R

pytestmark = pytest.mark.gpu
GUARD = 0x5a


def host(j, **caps):
    return SM.sam_host(SM.make_params(softclip=j["softclip"]), j["mode"], j["regs"], j["reg_off"], j["pairs"], j["alns"], j["cigar"], j["qer"],
                       j["read_off"], j["read_len"], j["qual"], j["names"], j["contig_names"], j["text"], j["L"], j["contig_off"], **caps)


def device(j, rec_cap=None, md_cap=None, text_cap=None, n_regs=None, slack=3):
    """gbx_mem_sam_device on the job's arrays.  The capacities of the inputs are `slack` above the counts, every output has guard
    bytes behind its capacity.  -> (result dict cut to the capacities, guards intact, the inputs unchanged)."""
    import torch
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    p = SM.make_params(softclip=j["softclip"])
    want = K.reference(j)
    n_reads, nr, na, nc = len(j["reg_off"]) - 1, len(j["regs"]), len(j["alns"]), len(j["cigar"])
    rcap = want["n_recs"] + slack if rec_cap is None else rec_cap
    mcap = want["n_md"] + slack if md_cap is None else md_cap
    tcap = want["n_text"] + slack if text_cap is None else text_cap
    nm, no = SM.arena(j["names"])
    cn, cno = SM.arena(j["contig_names"])
    pad = lambda a, n: np.concatenate([np.ascontiguousarray(a).view(np.uint8), np.zeros(n, np.uint8)])
    ins = [pad(j["regs"], slack * 88), j["reg_off"], pad(j["alns"], slack * 48), np.concatenate([j["cigar"], np.zeros(slack, np.uint32)]),
           np.array([nr if n_regs is None else n_regs, nc], np.int64), pad(j["qer"], 1), j["read_off"], j["read_len"], pad(nm, 1), no, pad(cn, 1), cno,
           j["contig_off"]]
    if j["pairs"] is not None:
        ins.append(pad(j["pairs"], 8))
    if j["qual"] is not None:
        ins.append(pad(j["qual"], 1))
    d = [t(a) for a in ins]
    d_rg, d_ro, d_al, d_cg, d_n, d_q, d_qo, d_ql, d_nm, d_no, d_cn, d_cno, d_co = d[:13]
    d_pa = d[13] if j["pairs"] is not None else None
    d_qu = d[-1] if j["qual"] is not None else None
    if "text_window" in j:                               # a text of 2 GB: zeros but for a window
        at, n = j["text_window"]
        d_tx = torch.zeros(len(j["text"]), dtype=torch.uint8, device=dev)
        d_tx[at:at + n] = t(j["text"][at:at + n])
    else:
        d_tx = t(j["text"])
    full = lambda n, size: torch.full(((n + 16) * size,), GUARD, dtype=torch.uint8, device=dev)
    d_rec, d_rof, d_md, d_li = full(rcap, 112), full(n_reads + 1, 8), full(mcap, 1), full(tcap, 1)
    d_out = torch.full((3,), -7, dtype=torch.int64, device=dev)
    wb = SM.lib().gbx_mem_sam_workspace_bytes(n_reads, nr + slack, na + slack)
    d_w = torch.empty(max(wb, 1), dtype=torch.uint8, device=dev)
    o = d_out.data_ptr()
    N.check(SM.lib().gbx_mem_sam_device(
        C.byref(p), n_reads, j["mode"], d_rg.data_ptr(), d_ro.data_ptr(), d_n.data_ptr(), nr + slack, d_pa.data_ptr() if d_pa is not None else None,
        d_al.data_ptr(), na + slack, d_cg.data_ptr(), d_n.data_ptr() + 8, nc + slack, d_q.data_ptr(), len(j["qer"]), d_qo.data_ptr(), d_ql.data_ptr(),
        d_qu.data_ptr() if d_qu is not None else None, d_nm.data_ptr(), d_no.data_ptr(), len(nm), d_cn.data_ptr(), d_cno.data_ptr(), len(cn),
        d_tx.data_ptr(), len(j["text"]), j["L"], len(j["contig_off"]) - 1, d_co.data_ptr(), d_rec.data_ptr(), rcap, d_rof.data_ptr(), o,
        d_md.data_ptr(), mcap, o + 8, d_li.data_ptr(), tcap, o + 16, d_w.data_ptr(), wb, None))
    torch.cuda.synchronize()
    n_r, n_m, n_t = (int(x) for x in d_out.cpu().numpy())
    rec, rof, md, li = (x.cpu().numpy() for x in (d_rec, d_rof, d_md, d_li))
    ur, um, ut = (min(max(n, 0), cap) for n, cap in ((n_r, rcap), (n_m, mcap), (n_t, tcap)))
    if n_r < 0:                                           # an overflow before the stage: the whole capacities are written (zeroed)
        ur, um, ut = rcap, mcap, tcap
    intact = bool((rec[ur * 112:] == GUARD).all() and (rof[(n_reads + 1) * 8:] == GUARD).all() and (md[um:] == GUARD).all() and
                  (li[ut:] == GUARD).all())
    unchanged = all(np.array_equal(x.cpu().numpy(), np.ascontiguousarray(a)) for x, a in zip(d, ins))
    out = dict(recs=rec[:ur * 112].view(SM.SAM_DTYPE), rec_off=rof[:(n_reads + 1) * 8].view(np.int64), n_recs=n_r, md=md[:um], n_md=n_m,
               lines=li[:ut], n_text=n_t)
    return out, intact, unchanged


def checked(j, w):
    assert R.validate(w["lines"].tobytes(), j["text"], j["contig_names"], j["contig_off"], w["recs"]) == w["n_recs"]


def both_entries(j):
    want = K.reference(j)
    got, intact, unchanged = device(j)
    assert intact and unchanged
    K.same(got, want)
    checked(j, got)
    h = host(j)
    K.same(h, want)
    checked(j, h)
    return want


@pytest.mark.parametrize("name", sorted(K.hand_built()))
def test_hand_built(name):
    w = both_entries(K.hand_built()[name])
    assert w["lines"].tobytes().decode("latin-1") == "".join(K.expected()[name])


def test_big_pos():
    """POS across 10^9: a text of 2 x (10^9 + 200) bytes."""
    w = both_entries(K.big_pos())
    assert w["lines"].tobytes().decode("latin-1") == K.expected()["big_pos"]


def test_capacity_one_short():
    j = K.hand_built()["three_records"]
    full = K.reference(j)
    need = dict(rec_cap=full["n_recs"], md_cap=full["n_md"], text_cap=full["n_text"])
    for which in need:
        for cap in (need[which] - 1, need[which]):
            caps = dict(need, **{which: cap})
            got, intact, unchanged = device(j, **caps)
            assert intact and unchanged
            K.same(got, K.reference(j, **caps))           # the counts report the need; the offsets in the records stay true
        with pytest.raises(N.GbxError) as e:
            host(j, **dict(need, **{which: need[which] - 1}))
        assert e.value.code == N.GBX_ERR_ARG and str(need[which]) in str(e.value)
    K.same(host(j, **need), full)


def test_upstream_overflow():
    j = K.hand_built()["tlen"]
    for n_regs in (-1, len(j["regs"]) + 4):
        got, intact, unchanged = device(j, n_regs=n_regs)
        assert intact and unchanged and (got["n_recs"], got["n_md"], got["n_text"]) == (-1, -1, -1)
        assert not got["rec_off"].any() and not got["recs"].tobytes().strip(b"\0") and not got["md"].any() and not got["lines"].any()
        assert len(got["lines"]) == K.reference(j)["n_text"] + 3


def test_two_runs_are_byte_equal():
    j = K.hand_built()["m_runs"]
    a, b = device(j)[0], device(j)[0]
    h1, h2 = host(j), host(j)
    for k in ("recs", "rec_off", "md", "lines"):
        assert a[k].tobytes() == b[k].tobytes() == h1[k].tobytes() == h2[k].tobytes()


def test_four_host_threads():
    jobs = [K.hand_built()[n] for n in ("m_runs", "three_records", "indels", "unmapped")]
    want = [K.reference(j) for j in jobs]
    host(jobs[0])
    got, err = [None] * 4, []

    def work(t):
        try:
            for _ in range(3):
                got[t] = host(jobs[t])
        except Exception as e:       # noqa: BLE001
            err.append(e)
    th = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not err, err
    for t in range(4):
        K.same(got[t], want[t])


def test_host_checks():
    j = K.hand_built()["three_records"]

    def bad(what, **kw):
        with pytest.raises(N.GbxError) as e:
            host(dict(j, **kw))
        assert e.value.code == N.GBX_ERR_ARG and what in str(e.value), str(e.value)
    bad("softclip", softclip=3)
    bad("mode", mode=-1)
    g = j["regs"].copy()
    g["sel"][[3, 6]] = -1
    bad("region 3: sel = -1", regs=g)
    a = j["alns"].copy()
    a["rid"][:] = -1
    bad("region 1: its alignment's rid = -1", alns=a)
    off = j["reg_off"].copy()
    off[-1] += 1
    bad("reg_off leaves the 7 regions", reg_off=off)
    # a reported region whose aln has rid < 0 is an unmapped record on the device
    got, intact, unchanged = device(dict(j, alns=a))
    assert intact and unchanged and got["n_recs"] == 5 and (got["recs"]["flag"] & 0x4).all() and (got["recs"]["n_cigar"] == 0).all()
    assert got["lines"].tobytes().count(b"\t*\t0\t0\t*\t*\t0\t0\t") == 5


def chimeric_pairs(g, n, seed, mean=300., sd=25.):
    """n FR pairs of 101-base reads cut from g, interleaved.  Every fifth pair has a mate with a substitution every 15 bases (no
    exact 19-mer: only the rescue finds it); every seventh pair's first read is chimeric: 50 bases from the fragment, 51 from
    another place on the other strand."""
    rng = np.random.default_rng(seed)
    reads = []
    while len(reads) < 2 * n:
        k = len(reads) // 2
        frag = max(150, int(round(rng.normal(mean, sd))))
        at = int(rng.integers(0, len(g) - frag))
        ends = [g[at:at + 101].copy(), KG.revcomp(g[at + frag - 101:at + frag])]
        if k % 5 == 4:
            ends[1][7::15] = (ends[1][7::15] + 1) % 4
        if k % 7 == 3:
            other = int(rng.integers(0, len(g) - 101))
            ends[0][50:] = KG.revcomp(g[other:other + 51])
        reads += ends
    return FM.FmiReadSet.fixed(np.array(reads, dtype=np.uint8))


def test_whole_pipeline_on_one_stream():
    """smem -> sal -> chain -> extend -> regs -> pestat -> rescue -> pair -> cigar -> sam on one stream on a random genome of 30 kb
    with mutated mates and chimeric reads.  The text is the restatement's on the stages' device output, every line passes the
    validator, supplementary records with SA tags occur, and the nine shared fields are mem_pair.sam_fields' rows."""
    import torch
    g = KR.genome(30_000, 8301)
    co = np.array([0, 14_000, 30_000], dtype=np.int64)
    cnames = ["first", "second_contig"]
    n_pairs, pair_id0 = 60, 500
    rs = chimeric_pairs(g, n_pairs, 8311)
    names = ["pair%d" % (k // 2) for k in range(2 * n_pairs)]
    qual = np.random.default_rng(8313).integers(33, 74, len(rs.enc)).astype(np.uint8)
    idx, smp = FM.build_index(g, sa_compx=3)
    text = MC.text_of(g)
    cap = 8000
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d = FM.DeviceFmi(idx, rs, torch.device("cuda:0"))
        d.set_sa(smp)
        front = Stages(d, text, len(g), co, caps=dict(pos_cap=cap)).queue(s.cuda_stream, last="extend")
        p = MG.make_params()
        z_bytes = 1000 * MG.lib().gbx_mem_cigar_record_z_bytes(C.byref(p), 101, 200)
        sam, (rg, rsc, pe, cg, sm) = SM.pipeline(front.extend, names, qual, cnames, s.cuda_stream, pair_id0, cigar_params=p, cigar_cap=8 * cap,
                                                 z_bytes=z_bytes)
    s.synchronize()
    assert int(d.n_pos.item()) <= cap and not d.overflow()
    res, (alns, cigar), got = pe.results(), cg.results(), sm.results()
    reg_off = rsc.results()["xreg_off"]
    want = R.sam_all(1, res["pregs"].view(K.REG_DTYPE), reg_off, res["pairs"], alns, cigar, rs.enc, rs.read_off, rs.read_len, qual, names, cnames, text, len(g),
                     co)
    K.same(got, want)
    head = "@SQ\tSN:first\tLN:14000\n@SQ\tSN:second_contig\tLN:16000\n"
    assert sam.decode("latin-1") == head + want["lines"].tobytes().decode("latin-1")
    assert R.validate(got["lines"].tobytes(), text, cnames, co, got["recs"]) == got["n_recs"]
    assert want["rows"] == MP.sam_fields(res["pairs"], res["pregs"], alns, cigar)
    flags = got["recs"]["flag"]
    n_sup = int(((flags & 0x800) != 0).sum())
    n_sa = int((got["recs"]["n_sa"] > 0).sum())
    assert n_sup >= 5 and n_sa > n_sup and got["lines"].tobytes().count(b"\tSA:Z:") == n_sa
    assert b"H" in b"".join(l.split(b"\t")[5] for l in got["lines"].tobytes().split(b"\n")[:-1])
    assert int(((flags & 0x2) != 0).sum()) >= 80 and got["n_recs"] == 2 * n_pairs + n_sup
