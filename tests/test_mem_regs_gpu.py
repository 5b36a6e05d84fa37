"""Alignment regions on the GPU (gbx_mem_regs_device / gbx_mem_regs_host), byte-exact against the restated rules of
tests/mem_regs_ref.py on the regions, reg_off, the counts and the CIGAR list with its zeroed tail.  No tolerance: the CPU test
asserts that no input used here has a mapq on a log() boundary."""
import ctypes as C
import threading

import numpy as np
import pytest

from genomicsbench_amd import _native as N
from genomicsbench_amd import bsw_seeds as BS
from genomicsbench_amd import fmi as FM
from genomicsbench_amd import mem_chain as MC
from genomicsbench_amd import mem_cigar as MG
from genomicsbench_amd import mem_regs as MR
import mem_chain_cases as KC
import mem_cigar_cases as KG
import mem_regs_cases as K
import mem_regs_ref as R

pytestmark = pytest.mark.gpu
GUARD = 0x5a


def host(j, **kw):
    return MR.regs_host(MR.make_params(**j["params"]), j["chains"], j["chain_off"], j["seeds"], j["res"], j["l_rep"], j["read_id0"], **kw)


def device(j, reg_cap=None, sel_cap=None, slack=7, counts=None):
    """gbx_mem_regs_device on the job's arrays.  The capacities of the inputs are `slack` above the counts (zeroed seeds with
    results of all -1 behind them), the outputs get 16 guard records behind their capacity.
    -> (result dict cut to the capacities, guards intact)."""
    import torch
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    n_reads, n_chains, n_seeds = len(j["l_rep"]), len(j["chains"]), len(j["seeds"])
    chain_cap, seed_cap = n_chains + slack, n_seeds + slack
    d_ch = t(np.concatenate([j["chains"], np.zeros(slack, R.CHAIN_DTYPE)]).view(np.uint8))
    d_sd = t(np.concatenate([j["seeds"], np.zeros(slack, R.SEED_DTYPE)]).view(np.uint8))
    d_rs = t(np.concatenate([j["res"], np.full((slack, 8), -1, np.int32)]))
    d_cnt = t(np.array(counts if counts is not None else [n_chains, n_seeds], np.int64))
    d_co, d_lr = t(j["chain_off"]), t(np.concatenate([j["l_rep"], [0]]).astype(np.int32))
    rcap = seed_cap if reg_cap is None else reg_cap
    scap = seed_cap if sel_cap is None else sel_cap
    d_rg = torch.full(((rcap + 16) * 88,), GUARD, dtype=torch.uint8, device=dev)
    d_ss = torch.full(((scap + 16) * 40,), GUARD, dtype=torch.uint8, device=dev)
    d_sr = torch.full(((scap + 16) * 32,), GUARD, dtype=torch.uint8, device=dev)
    d_ro = torch.full((n_reads + 1,), -7, dtype=torch.int64, device=dev)
    d_out = torch.full((2,), -7, dtype=torch.int64, device=dev)
    wb = MR.lib().gbx_mem_regs_workspace_bytes(n_reads, seed_cap)
    d_w = torch.empty(max(wb, 1), dtype=torch.uint8, device=dev)
    p = MR.make_params(**j["params"])
    N.check(MR.lib().gbx_mem_regs_device(C.byref(p), n_reads, j["read_id0"], d_ch.data_ptr(), d_cnt.data_ptr(), chain_cap, d_co.data_ptr(),
                                         d_sd.data_ptr(), d_cnt.data_ptr() + 8, seed_cap, d_rs.data_ptr(), d_lr.data_ptr(),
                                         d_rg.data_ptr(), rcap, d_ro.data_ptr(), d_out.data_ptr(), d_ss.data_ptr(), d_sr.data_ptr(), scap,
                                         d_out.data_ptr() + 8, d_w.data_ptr(), wb, None))
    torch.cuda.synchronize()
    nr, ns = (int(x) for x in d_out.cpu().numpy())
    rg, ss, sr = d_rg.cpu().numpy(), d_ss.cpu().numpy(), d_sr.cpu().numpy()
    intact = bool((rg[rcap * 88:] == GUARD).all() and (ss[scap * 40:] == GUARD).all() and (sr[scap * 32:] == GUARD).all())
    out = dict(regs=rg[:max(0, min(nr, rcap)) * 88].view(MR.REG_DTYPE), reg_off=d_ro.cpu().numpy(), n_regs=nr, n_sel=ns,
               sel_seeds=ss[:scap * 40].view(BS.SEED_DTYPE), sel_res=sr[:scap * 32].view(np.int32).reshape(-1, 8))
    return out, intact


def both_entries(j):
    n = len(j["seeds"])
    got, ok = device(j)
    assert ok
    K.same(got, K.reference(j, sel_cap=n + 7))
    want = K.reference(j)
    K.same(host(j), want)
    return want


@pytest.mark.parametrize("name", sorted(K.hand_built()))
def test_hand_built_cases(name):
    both_entries(K.hand_built()[name])


def test_reads_that_straddle_the_wave_width():
    """0, 1, 2, 63, 64, 65 and 130 regions in a read (130 of them primaries: z passes 64), chains of 100 and 200 seeds, a dedup
    over 74 regions."""
    j = K.straddle()
    want = both_entries(j)
    assert np.diff(want["reg_off"]).tolist()[:9] == [0, 1, 2, 63, 64, 65, 130, 70, 130]
    assert int(j["chains"]["n_seeds"].max()) == 200


@pytest.mark.parametrize("n_reads", [1, 2, 300])
def test_generated_reads(n_reads):
    both_entries(K.synthetic(n_reads, 21))
    if n_reads == 300:
        both_entries(K.synthetic(300, 22, read_id0=5000))


def test_capacity_one_short():
    j = K.synthetic(300, 21)
    want = K.reference(j)
    nr, ns = want["n_regs"], want["n_sel"]
    assert nr > 300 and 100 < ns < nr
    for rcap, scap in ((nr - 1, None), (None, ns - 1), (0, 0), (nr, ns)):
        got, ok = device(j, rcap, scap)
        assert ok and (got["n_regs"], got["n_sel"]) == (nr, ns)       # the counts report the need; the guards survive
        assert np.array_equal(got["reg_off"], want["reg_off"])
        assert got["regs"].tobytes() == want["regs"][:len(got["regs"])].tobytes()      # reg.sel keeps the true index
        cut = K.reference(j, sel_cap=len(got["sel_seeds"]))
        assert got["sel_seeds"].tobytes() == cut["sel_seeds"].tobytes() and got["sel_res"].tobytes() == cut["sel_res"].tobytes()
    for kw in (dict(reg_cap=nr - 1), dict(sel_cap=ns - 1)):
        with pytest.raises(N.GbxError) as e:
            host(j, **kw)
        assert e.value.code == N.GBX_ERR_ARG and str(nr) in str(e.value) and str(ns) in str(e.value)
    K.same(host(j, reg_cap=nr, sel_cap=ns), K.reference(j, sel_cap=ns))


def test_upstream_overflow():
    j = K.synthetic(20, 23)
    n_chains, n_seeds = len(j["chains"]), len(j["seeds"])
    for counts in ([n_chains + 8, n_seeds], [n_chains, n_seeds + 8]):
        got, ok = device(j, counts=counts)
        assert ok and got["n_regs"] == -1 and got["n_sel"] == -1 and (got["reg_off"] == 0).all()
        assert (got["sel_res"] == -1).all() and not got["sel_seeds"].tobytes().strip(b"\0")


def test_two_runs_are_byte_equal():
    j = K.straddle()
    a, b = device(j)[0], device(j)[0]
    h1, h2 = host(j), host(j)
    for k in ("regs", "reg_off", "sel_seeds", "sel_res"):
        assert a[k].tobytes() == b[k].tobytes() and h1[k].tobytes() == h2[k].tobytes()
    assert a["regs"].tobytes() == h1["regs"].tobytes()


def test_four_host_threads():
    jobs = [K.synthetic(150, 40 + t, read_id0=1000 * t) for t in range(4)]
    want = [K.reference(j) for j in jobs]
    assert all(w["boundary"] == 0 for w in want)
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


def pipeline_reads(g, n, seed):
    """n reads of 151 bases cut from g, both strands, with substitutions and short indels (mem_cigar_cases.mutate)."""
    rng = np.random.default_rng(seed)
    reads = []
    for _ in range(n):
        at = int(rng.integers(0, len(g) - 160))
        piece = g[at:at + 159]
        subs = set(int(x) for x in rng.integers(0, 151, int(rng.integers(0, 4))))
        ins = set(int(x) for x in rng.integers(30, 120, 1)) if rng.random() < 0.3 else set()
        dele = set(int(x) for x in rng.integers(30, 120, int(rng.integers(1, 3)))) if rng.random() < 0.3 else set()
        rd = KG.mutate(piece, subs, ins, dele)[:151]
        reads.append(KG.revcomp(rd) if rng.random() < 0.5 else rd)
    return FM.FmiReadSet.fixed(np.array(reads, dtype=np.uint8))


def test_whole_pipeline_on_one_stream():
    """smem -> sal -> chain -> extend -> regs -> cigar queued back to back on one stream, no count read in between, one
    synchronise at the end; against the references chained on the CPU (mem_chain_ref, the seed extension's host entry, which
    test_bsw_seeds_gpu pins, mem_regs_ref, mem_cigar_ref).  The genome has a planted repeat, so some reads have two loci."""
    import torch
    from genomicsbench_amd.datagen import gen_fmi_genome
    g = gen_fmi_genome(20_000, 8101)
    g[15_000:15_600] = g[3_000:3_600]                 # the planted repeat
    g[15_100], g[15_300], g[15_500] = (g[15_100] + 1) % 4, (g[15_300] + 2) % 4, (g[15_500] + 1) % 4
    co = np.array([0, 9_000, 20_000], dtype=np.int64)
    rs = pipeline_reads(g, 200, 8102)
    for k, at in enumerate((3_100, 3_300, 15_200)):   # three reads inside the repeat
        rs.enc[rs.read_off[k]:rs.read_off[k] + 151] = g[at:at + 151]
    idx, smp = FM.build_index(g, sa_compx=3)
    text = MC.text_of(g)
    sp = BS.make_seed_params()
    cap = 12000
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d = FM.DeviceFmi(idx, rs, torch.device("cuda:0"))
        d.set_sa(smp)
        d.run(s.cuda_stream)
        d.sal(500, pos_cap=cap, stream=s.cuda_stream)
        mc = MC.DeviceMemChain(d, len(g), co)
        mc.run(s.cuda_stream)
        ext = mc.extension(text)
        ext.run(sp, s.cuda_stream)
        rg = MR.DeviceMemRegs(ext, read_id0=77)
        rg.run(s.cuda_stream)
        p = MG.make_params()
        z_bytes = 600 * MG.lib().gbx_mem_cigar_record_z_bytes(C.byref(p), 151, 200)
        cg = MG.DeviceMemCigar(rg.cigar_input, p, cigar_cap=8 * cap, z_bytes=z_bytes)
        assert cg.n == rg.sel_cap == mc.seed_cap == cap
        cg.run(s.cuda_stream)
    s.synchronize()
    assert int(d.n_pos.item()) <= cap and not d.overflow()
    # the references, chained
    smems, smem_off = FM.smem_host(idx, rs)
    pos, pos_off = FM.sal_host(idx, smp, smems, 500)
    jc = dict(m=smems["m"].astype(np.int64), n=smems["n"].astype(np.int64), s=smems["s"], smem_off=smem_off, pos=pos, pos_off=pos_off,
              read_off=rs.read_off, read_len=rs.read_len, L=len(g), contig_off=co, params={})
    wc = KC.reference(jc)
    KC.same(mc.results(), wc)
    n_seeds = len(wc["seeds"])
    assert 200 <= n_seeds < cap
    res = BS.extend_seeds_host(sp, BS.SeedBatch(text, rs.enc, wc["seeds"]))
    assert np.array_equal(ext.results()[:n_seeds], res)
    wr = R.regs_all(wc["chains"], wc["chain_off"], wc["seeds"], res, wc["l_rep"], R.params(), 77, sel_cap=cap)
    assert wr["boundary"] == 0
    got = rg.results()
    K.same(got, wr)
    n_sel = wr["n_sel"]
    assert 150 <= n_sel < wr["n_regs"] < n_seeds and (wr["regs"]["secondary"] >= 0).any()
    jg = dict(params={}, L=len(g), contig_off=co, text=text, qer=rs.enc, seeds=wr["sel_seeds"], res=wr["sel_res"])
    want = KG.reference_c(jg)
    alns, cigar = cg.results()
    KG.same((alns, cigar), want)
    assert (alns["rid"][:n_sel] >= 0).all() and (alns["rid"][n_sel:] == -1).all()      # it aligned exactly n_sel records
    rows = MR.alignments(got["regs"], alns, cigar)
    assert len(rows) == n_sel and {r[0] for r in rows} <= set(range(200))
    inside = [r for r in rows if r[0] < 3]
    assert len(inside) == 3 and all(r[4] < 60 and r[6] == "151M" for r in inside)      # a read inside the repeat: one alignment, low mapq
    assert sum(1 for r in rows if r[4] == 60) > 100
