"""Paired-end on the GPU (gbx_mem_pair_device / gbx_mem_pair_host), byte-exact against the restated rules of
tests/mem_pair_ref.py on the estimate, the pair records, the regions, the count and the new CIGAR list with its zeroed tail.  No
tolerance: the CPU test asserts that no input used here is a boundary input."""
import ctypes as C
import threading

import numpy as np
import pytest

from genomicsbench_amd import _native as N
from genomicsbench_amd import bsw_seeds as BS
from genomicsbench_amd import fmi as FM
from genomicsbench_amd import mem_chain as MC
from genomicsbench_amd import mem_cigar as MG
from genomicsbench_amd import mem_pair as MP
from genomicsbench_amd import mem_regs as MR
import mem_chain_cases as KC
import mem_cigar_cases as KG
import mem_pair_cases as K
import mem_pair_ref as R
import mem_regs_cases as KR
import mem_regs_ref as RR

pytestmark = pytest.mark.gpu
GUARD = 0x5a


def host(j, **kw):
    return MP.pair_host(MP.make_params(**j["params"]), j["regs"], j["reg_off"], j["sel_seeds"], j["sel_res"], j["seeds"], j["l_rep"], j["L"],
                        j["contig_off"], j["pair_id0"], j["pes_in"], **kw)


def device(j, psel_cap=None, slack=5, n_regs=None):
    """gbx_mem_pair_device on the job's arrays.  The capacities of the inputs are `slack` above the counts, the outputs get 16
    guard records behind their capacity.  -> (result dict cut to the capacities, guards intact, the inputs unchanged)."""
    import torch
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    nr, ns, nsd, n_pairs = len(j["regs"]), len(j["sel_seeds"]), len(j["seeds"]), (len(j["reg_off"]) - 1) // 2
    reg_cap, sel_cap, seed_cap = nr + slack, ns + slack, nsd + slack
    ins = [np.concatenate([j["regs"], np.zeros(slack, RR.REG_DTYPE)]).view(np.uint8), j["reg_off"],
           np.concatenate([j["sel_seeds"], np.zeros(slack, RR.SEED_DTYPE)]).view(np.uint8),
           np.concatenate([j["sel_res"], np.full((slack, 8), -1, np.int32)]), np.concatenate([j["seeds"], np.zeros(slack, RR.SEED_DTYPE)]).view(np.uint8),
           np.concatenate([j["l_rep"], [0]]).astype(np.int32), j["contig_off"], np.array([nr if n_regs is None else n_regs], np.int64)]
    d_rg, d_ro, d_ss, d_sr, d_sd, d_lr, d_co, d_n = (t(a) for a in ins)
    pcap = reg_cap if psel_cap is None else psel_cap
    d_pe = torch.full((4 * 32,), GUARD, dtype=torch.uint8, device=dev)
    d_pa = torch.full(((n_pairs + 16) * 56,), GUARD, dtype=torch.uint8, device=dev)
    d_pr = torch.full(((reg_cap + 16) * 88,), GUARD, dtype=torch.uint8, device=dev)
    d_ps = torch.full(((pcap + 16) * 40,), GUARD, dtype=torch.uint8, device=dev)
    d_pq = torch.full(((pcap + 16) * 32,), GUARD, dtype=torch.uint8, device=dev)
    d_out = torch.full((1,), -7, dtype=torch.int64, device=dev)
    p = MP.make_params(**j["params"])
    wb = MP.lib().gbx_mem_pair_workspace_bytes(n_pairs, reg_cap, p.max_ins)
    d_w = torch.empty(max(wb, 1), dtype=torch.uint8, device=dev)
    given = MP.pestat_records(j["pes_in"])
    N.check(MP.lib().gbx_mem_pair_device(C.byref(p), n_pairs, j["pair_id0"], d_rg.data_ptr(), d_ro.data_ptr(), d_n.data_ptr(), reg_cap,
                                         d_ss.data_ptr(), d_sr.data_ptr(), sel_cap, d_sd.data_ptr(), seed_cap, d_lr.data_ptr(), j["L"],
                                         len(j["contig_off"]) - 1, d_co.data_ptr(), N.ptr(given), d_pe.data_ptr(), d_pa.data_ptr(),
                                         d_pr.data_ptr(), d_ps.data_ptr(), d_pq.data_ptr(), pcap, d_out.data_ptr(), d_w.data_ptr(), wb, None))
    torch.cuda.synchronize()
    n = int(d_out.item())
    pa, pr, ps, pq = d_pa.cpu().numpy(), d_pr.cpu().numpy(), d_ps.cpu().numpy(), d_pq.cpu().numpy()
    used = nr if n >= 0 else 0
    intact = bool((pa[n_pairs * 56:] == GUARD).all() and (pr[used * 88:] == GUARD).all() and (ps[pcap * 40:] == GUARD).all() and
                  (pq[pcap * 32:] == GUARD).all())
    unchanged = all(np.array_equal(d.cpu().numpy(), np.ascontiguousarray(a)) for d, a in zip((d_rg, d_ro, d_ss, d_sr, d_sd, d_lr, d_co, d_n), ins))
    out = dict(pes=d_pe.cpu().numpy().view(MP.PESTAT_DTYPE), pairs=pa[:n_pairs * 56].view(MP.PAIR_DTYPE), pregs=pr[:used * 88].view(MP.REG_DTYPE),
               psel_seeds=ps[:pcap * 40].view(BS.SEED_DTYPE), psel_res=pq[:pcap * 32].view(np.int32).reshape(-1, 8), n_psel=n)
    return out, intact, unchanged


def both_entries(j):
    got, intact, unchanged = device(j)
    assert intact and unchanged
    K.same(got, K.reference(j, psel_cap=len(j["regs"]) + 5))
    want = K.reference(j)
    K.same(host(j), want)
    return want


@pytest.mark.parametrize("name", sorted(K.hand_built()))
def test_hand_built_cases(name):
    both_entries(K.hand_built()[name])


@pytest.mark.parametrize("name", ["one", "two", "many", "many_id0", "given"])
def test_generated_pairs(name):
    want = both_entries(K.gpu_inputs()[name])
    if name == "many":
        assert want["pes"]["failed"].tolist() == [0, 0, 0, 1] and want["pairs"]["proper"].sum() > 250


def test_pairs_that_straddle_the_wave_width():
    """63, 64, 65 and 200 keys in a pair (the register sort, its edge, the bitonic network) and a look-back over 90 keys before
    `high` ends it."""
    want = both_entries(K.gpu_inputs()["straddle"])
    assert want["pairs"]["n_cand"].max() > 1000 and want["pairs"]["n_cand"][4] == 6


@pytest.mark.parametrize("name", ["max_ins_1", "max_ins_2_20"])
def test_max_ins_at_its_ends(name):
    want = both_entries(K.gpu_inputs()[name])
    assert want["pes"]["failed"].tolist() == ([0, 1, 1, 1] if name == "max_ins_1" else [1, 0, 1, 1])


def test_capacity_one_short():
    j = K.gpu_inputs()["many"]
    want = K.reference(j)
    n = want["n_psel"]
    assert n > len(j["sel_seeds"]) > 300                             # the new list is longer than the regs stage's here
    for cap in (n - 1, 0, n):
        got, intact, unchanged = device(j, psel_cap=cap)
        assert intact and unchanged and got["n_psel"] == n           # the count reports the need; the guards survive
        cut = K.reference(j, psel_cap=cap)
        K.same(got, cut)                                              # reg.sel keeps the true index
    with pytest.raises(N.GbxError) as e:
        host(j, psel_cap=n - 1)
    assert e.value.code == N.GBX_ERR_ARG and str(n) in str(e.value)
    K.same(host(j, psel_cap=n), K.reference(j, psel_cap=n))


def test_upstream_overflow():
    j = K.gpu_inputs()["given"]
    for n_regs in (-1, len(j["regs"]) + 6):
        got, intact, unchanged = device(dict(j, pes_in=None), n_regs=n_regs)
        assert intact and unchanged and got["n_psel"] == -1
        assert not got["pairs"].tobytes().strip(b"\0") and got["pes"]["failed"].tolist() == [1, 1, 1, 1]
        assert (got["psel_res"] == -1).all() and not got["psel_seeds"].tobytes().strip(b"\0")


def test_two_runs_are_byte_equal():
    j = K.gpu_inputs()["many"]
    a, b = device(j)[0], device(j)[0]
    h1, h2 = host(j), host(j)
    for k in ("pes", "pairs", "pregs", "psel_seeds", "psel_res"):
        assert a[k].tobytes() == b[k].tobytes() and h1[k].tobytes() == h2[k].tobytes()
    assert a["pregs"].tobytes() == h1["pregs"].tobytes() and a["pes"].tobytes() == h1["pes"].tobytes()


def test_four_host_threads():
    jobs = [K.gpu_inputs()["thread%d" % t] for t in range(4)]
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


def pipeline_pairs(g, n, seed, mean=300., sd=25.):
    """n FR pairs of 101-base reads cut from g, interleaved: the first read forward at the fragment's start, its mate the
    reverse complement of the fragment's end, each with a few substitutions; every 16th pair is turned round as a whole."""
    rng = np.random.default_rng(seed)
    reads = []
    for k in range(n):
        frag = max(150, int(round(rng.normal(mean, sd))))
        at = int(rng.integers(0, len(g) - frag))
        ends = [g[at:at + 101].copy(), KG.revcomp(g[at + frag - 101:at + frag])]
        for rd in ends:
            for x in rng.integers(0, 101, int(rng.integers(0, 3))):
                rd[x] = (rd[x] + 1) % 4
        if k % 16 == 15:
            ends = ends[::-1]
        reads += ends
    return FM.FmiReadSet.fixed(np.array(reads, dtype=np.uint8))


def test_whole_pipeline_on_one_stream():
    """smem -> sal -> chain -> extend -> regs (read_id0 = 2 pair_id0) -> pair -> cigar queued back to back on one stream, no count
    read in between, one synchronise at the end; against the references chained on the CPU (mem_chain_ref, the seed extension's
    host entry, mem_regs_ref, mem_pair_ref, mem_cigar_ref).  Every simulated pair is an FR fragment on a genome without repeats,
    so all of them should pair; reads that fall on a contig boundary or lose an end may not: at least 90 % proper is asserted, and
    the device's share is the reference's, which the comparison fixes."""
    import torch
    from genomicsbench_amd.datagen import gen_fmi_genome
    g = gen_fmi_genome(30_000, 8301)
    co = np.array([0, 14_000, 30_000], dtype=np.int64)
    n_pairs, pair_id0 = 200, 500
    rs = pipeline_pairs(g, n_pairs, 8302)
    idx, smp = FM.build_index(g, sa_compx=3)
    text = MC.text_of(g)
    sp = BS.make_seed_params()
    cap = 24000
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
        rg = MR.DeviceMemRegs(ext, read_id0=2 * pair_id0)
        rg.run(s.cuda_stream)
        pe = MP.DeviceMemPair(rg)
        pe.run(s.cuda_stream)
        p = MG.make_params()
        z_bytes = 1000 * MG.lib().gbx_mem_cigar_record_z_bytes(C.byref(p), 101, 200)
        cg = MG.DeviceMemCigar(pe.cigar_input, p, cigar_cap=8 * cap, z_bytes=z_bytes)
        assert cg.n == pe.psel_cap == rg.sel_cap == cap
        cg.run(s.cuda_stream)
    s.synchronize()
    assert int(d.n_pos.item()) <= cap and not d.overflow()
    # the references, chained
    smems, smem_off = FM.smem_host(idx, rs)
    pos, pos_off = FM.sal_host(idx, smp, smems, 500)
    jc = dict(m=smems["m"].astype(np.int64), n=smems["n"].astype(np.int64), s=smems["s"], smem_off=smem_off, pos=pos, pos_off=pos_off,
              read_off=rs.read_off, read_len=rs.read_len, L=len(g), contig_off=co, params={})
    wc = KC.reference(jc)
    res = BS.extend_seeds_host(sp, BS.SeedBatch(text, rs.enc, wc["seeds"]))
    wr = RR.regs_all(wc["chains"], wc["chain_off"], wc["seeds"], res, wc["l_rep"], RR.params(), 2 * pair_id0, sel_cap=cap)
    assert wr["boundary"] == 0
    KR.same(rg.results(), wr)
    wp = R.pair_all(wr["regs"], wr["reg_off"], wr["sel_seeds"], wr["sel_res"], wc["seeds"], wc["l_rep"], len(g), co, R.params(), pair_id0,
                    psel_cap=cap)
    assert wp["boundary"] == 0, wp["notes"][:3]
    got = pe.results()
    K.same(got, wp)
    assert not wp["pes"]["failed"][1] and 250 < wp["pes"]["avg"][1] < 350
    assert wp["pairs"]["proper"].sum() >= 0.9 * n_pairs and wp["pairs"]["paired"].sum() >= 0.9 * n_pairs
    n_sel = wp["n_psel"]
    jg = dict(params={}, L=len(g), contig_off=co, text=text, qer=rs.enc, seeds=wp["psel_seeds"], res=wp["psel_res"])
    want = KG.reference_c(jg)
    alns, cigar = cg.results()
    KG.same((alns, cigar), want)
    assert (alns["rid"][:n_sel] >= 0).all() and (alns["rid"][n_sel:] == -1).all()
    rows = MP.sam_fields(got["pairs"], got["pregs"], alns, cigar)
    assert {r[0] for r in rows} == set(range(2 * n_pairs))
    proper = [r for r in rows if r[1] & 0x2]
    assert len(proper) >= 2 * 0.9 * n_pairs and all(r[2] == r[6] and 150 <= abs(r[8]) <= 450 for r in proper)
