"""Seed chaining on the GPU (gbx_mem_chain_device / gbx_mem_chain_host), bit-exact against the restated rules of
tests/mem_chain_ref.py on chains, chain_off, seeds and l_rep."""
import ctypes as C
import threading

import numpy as np
import pytest

from genomicsbench_amd import _native as N
from genomicsbench_amd import bsw_seeds as BS
from genomicsbench_amd import fmi as FM
from genomicsbench_amd import mem_chain as MC
from genomicsbench_amd.datagen import gen_fmi_genome, gen_fmi_reads
import mem_chain_cases as K

pytestmark = pytest.mark.gpu
GUARD = 0x5a


def smem_records(j):
    sm = np.zeros(len(j["m"]), dtype=FM.SMEM_DTYPE)
    sm["m"], sm["n"], sm["s"] = j["m"], j["n"], j["s"]
    return sm


def read_set(j):
    return FM.FmiReadSet(np.zeros(int(j["read_off"][-1] + j["read_len"][-1]) if len(j["read_len"]) else 0, np.uint8), j["read_off"], j["read_len"])


def host(j, **kw):
    return MC.chain_host(MC.make_params(**j["params"]), smem_records(j), j["smem_off"], j["pos"], j["pos_off"], read_set(j), j["L"],
                         j["contig_off"], **kw)


def device(j, chain_cap=None, seed_cap=None, slack=7):
    """gbx_mem_chain_device on the job's arrays.  The capacities of the inputs are `slack` above the counts, the outputs get
    16 guard records behind their capacity.  -> (result dict cut to the capacities, n_chains, n_seeds, guards intact)."""
    import torch
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    sm = smem_records(j)
    n_reads, n_smem, n_pos = len(j["read_len"]), len(sm), len(j["pos"])
    smem_cap, pos_cap = n_smem + slack, n_pos + slack
    d_sm = t(np.concatenate([sm, np.zeros(slack, FM.SMEM_DTYPE)]).view(np.uint8))
    d_pos = t(np.concatenate([j["pos"], np.full(slack, -7, np.int64)]))
    d_pos_off = t(np.concatenate([j["pos_off"], np.full(slack, n_pos, np.int64)]))
    d_cnt = t(np.array([n_smem, n_pos], np.int64))
    d_smem_off, d_ro, d_rl, d_co = t(j["smem_off"]), t(j["read_off"]), t(j["read_len"]), t(j["contig_off"])
    ccap = n_pos if chain_cap is None else chain_cap
    scap = n_pos if seed_cap is None else seed_cap
    d_ch = torch.full(((ccap + 16) * 56,), GUARD, dtype=torch.uint8, device=dev)
    d_sd = torch.full(((scap + 16) * 40,), GUARD, dtype=torch.uint8, device=dev)
    d_choff = torch.zeros(n_reads + 1, dtype=torch.int64, device=dev)
    d_lrep = torch.zeros(max(n_reads, 1), dtype=torch.int32, device=dev)
    d_out = torch.zeros(2, dtype=torch.int64, device=dev)
    wb = MC.lib().gbx_mem_chain_workspace_bytes(n_reads, smem_cap, pos_cap)
    d_w = torch.empty(max(wb, 1), dtype=torch.uint8, device=dev)
    p = MC.make_params(**j["params"])
    N.check(MC.lib().gbx_mem_chain_device(C.byref(p), n_reads, d_sm.data_ptr(), d_cnt.data_ptr(), smem_cap, d_smem_off.data_ptr(),
                                          d_pos.data_ptr(), d_cnt.data_ptr() + 8, pos_cap, d_pos_off.data_ptr(), d_ro.data_ptr(),
                                          d_rl.data_ptr(), int(j["L"]), len(j["contig_off"]) - 1, d_co.data_ptr(), d_ch.data_ptr(), ccap,
                                          d_choff.data_ptr(), d_sd.data_ptr(), scap, d_lrep.data_ptr(), d_out.data_ptr(),
                                          d_out.data_ptr() + 8, d_w.data_ptr(), wb, None))
    torch.cuda.synchronize()
    nc, ns = (int(x) for x in d_out.cpu().numpy())
    ch, sd = d_ch.cpu().numpy(), d_sd.cpu().numpy()
    intact = bool((ch[ccap * 56:] == GUARD).all() and (sd[scap * 40:] == GUARD).all())
    tail_zero = bool((sd[min(ns, scap) * 40:scap * 40] == 0).all())
    out = dict(chains=ch[:min(nc, ccap) * 56].view(MC.CHAIN_DTYPE), seeds=sd[:min(ns, scap) * 40].view(BS.SEED_DTYPE),
               chain_off=d_choff.cpu().numpy(), l_rep=d_lrep.cpu().numpy()[:n_reads])
    return out, nc, ns, intact and tail_zero


def both_entries(j, want=None):
    want = want or K.reference(j)
    got, nc, ns, ok = device(j)
    assert ok and nc == len(want["chains"]) and ns == len(want["seeds"])
    K.same(got, want)
    K.same(host(j), want)
    return want


@pytest.mark.parametrize("name", sorted(K.hand_built()))
def test_hand_built_hits(name):
    j = K.hand_built()[name]
    want = both_entries(j)
    if name == "filter":
        a, b = want["chain_off"][2], want["chain_off"][3]
        assert want["made"][2] == 3 and want["chains"][a:b]["kept"].tolist() == [3, 1]       # the reference drops the third
    if name == "tie":
        assert want["made"] == [2, 3]
    if name.startswith("max_chain_extend"):
        assert len(K.reference(j, max_chain_extend=1 << 30)["chains"]) > len(want["chains"]) or name.endswith("2")


def test_synthetic_hits_many_chains_and_contigs():
    for j in (K.synthetic(300, 11, many=(5, 77)), K.synthetic(200, 12, L=9000, contig_off=[0, 700, 760, 4000, 9000], many=(9,))):
        want = both_entries(j)
        assert max(want["made"]) > 64 and (want["l_rep"] > 0).any()


@pytest.fixture(scope="module")
def small():
    g = gen_fmi_genome(60_000, 6101)
    rs = gen_fmi_reads(g, 2000, 6102)
    return g, rs


def fmi_inputs(g, rs, cx, max_occ):
    idx, smp = FM.build_index(g, sa_compx=cx)
    smems, smem_off = FM.smem_host(idx, rs)
    pos, pos_off = FM.sal_host(idx, smp, smems, max_occ)
    j = dict(m=smems["m"].astype(np.int64), n=smems["n"].astype(np.int64), s=smems["s"], smem_off=smem_off, pos=pos, pos_off=pos_off,
             read_off=rs.read_off, read_len=rs.read_len, L=len(g), contig_off=MC.one_contig(len(g)), params=dict(max_occ=max_occ))
    return idx, smp, smems, j


def device_pipeline(idx, smp, rs, j, stream=None, ext_params=None, text=None):
    import torch
    d = FM.DeviceFmi(idx, rs, torch.device("cuda:0"))
    d.set_sa(smp)
    s = stream.cuda_stream if stream is not None else None
    d.run(s)
    d.sal(j["params"]["max_occ"], pos_cap=len(j["pos"]) + 100, stream=s)
    mc = MC.DeviceMemChain(d, j["L"], j["contig_off"], MC.make_params(**j["params"]))
    mc.run(s)
    ext = None
    if ext_params is not None:
        ext = mc.extension(text, n=min(mc.seed_cap, 60_000))
        ext.run(ext_params, s)
    return d, mc, ext


@pytest.mark.parametrize("cx", [0, 3])
def test_reads_of_the_generator(small, cx):
    import torch
    g, rs = small
    idx, smp, smems, j = fmi_inputs(g, rs, cx, 500)
    assert len(smems) > 2000
    want = K.reference(j)
    K.same(host(j), want)
    d, mc, _ = device_pipeline(idx, smp, rs, j)
    torch.cuda.synchronize()
    K.same(mc.results(), want)


def repetitive():
    rng = np.random.default_rng(5)
    elem = rng.integers(0, 4, 700).astype(np.uint8)
    parts = []
    for _ in range(80):
        c = elem.copy()
        hit = rng.random(700) < 0.02
        c[hit] = (c[hit] + 1) % 4
        parts += [c, rng.integers(0, 4, int(rng.integers(5, 60))).astype(np.uint8)]
    g = np.concatenate(parts)
    reads = []
    for _ in range(60):
        p = int(rng.integers(0, len(g) - 151))
        r = g[p:p + 151].copy()
        if rng.random() < 0.5:
            r = 3 - r[::-1]
        hit = rng.random(151) < 0.015
        r[hit] = (r[hit] + 1) % 4
        reads.append(r)
    return g, FM.FmiReadSet.fixed(np.array(reads))


@pytest.mark.parametrize("max_occ", [4, 500])
def test_repeats(max_occ):
    import torch
    g, rs = repetitive()
    idx, smp, smems, j = fmi_inputs(g, rs, 3, max_occ)
    want = K.reference(j)
    if max_occ == 4:
        assert int(smems["s"].max()) > 4 and (want["l_rep"] > 0).any()
    else:
        assert max(want["made"]) > 64            # the register sort ends at 64 chains: such reads take the slab's network
    K.same(host(j), want)
    d, mc, _ = device_pipeline(idx, smp, rs, j)
    torch.cuda.synchronize()
    K.same(mc.results(), want)


def test_chained_on_one_stream_without_a_host_sync():
    """smem, sal, chain and extension queued back to back on one stream, one synchronise at the end."""
    import torch
    g = gen_fmi_genome(60_000, 6101)
    rs = gen_fmi_reads(g, 300, 6103)
    exact = [5, 17, 250]
    for k, r in enumerate(exact):                     # exact copies of the genome, forward and reverse strand
        piece = g[1000 + 997 * k:1000 + 997 * k + 151]
        rs.enc[rs.read_off[r]:rs.read_off[r] + 151] = piece if k != 1 else 3 - piece[::-1]
    idx, smp, smems, j = fmi_inputs(g, rs, 3, 500)
    want = K.reference(j)
    sp = BS.make_seed_params()
    text = MC.text_of(g)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d, mc, ext = device_pipeline(idx, smp, rs, j, s, sp, text)
    s.synchronize()
    K.same(mc.results(), want)
    n = len(want["seeds"])
    assert 0 < n < ext.n
    got = ext.results()
    ref = BS.extend_seeds_host(sp, BS.SeedBatch(text, rs.enc, want["seeds"]))
    assert np.array_equal(got[:n], ref)
    assert (got[n:] == -1).all()                      # the zeroed records past the count are no seeds
    F = {f: k for k, f in enumerate(BS.SEED_RESULT_FIELDS)}
    for r in exact:
        c0, c1 = want["chain_off"][r], want["chain_off"][r + 1]
        assert c1 > c0
        best = want["chains"][c0]
        assert best["weight"] == 151
        for k in range(best["seed_off"], best["seed_off"] + best["n_seeds"]):
            assert got[k, F["qb"]] == 0 and got[k, F["qe"]] == 151 and got[k, F["truesc"]] == 151 * sp.bsw.mat[0]


def test_capacity():
    j = K.synthetic(60, 21)
    want = K.reference(j)
    nc, ns = len(want["chains"]), len(want["seeds"])
    assert nc > 20 and ns > nc
    for ccap, scap in ((nc - 3, None), (None, ns - 5), (0, 0), (nc, ns)):
        got, gc, gs, ok = device(j, ccap, scap)
        assert (gc, gs) == (nc, ns) and ok           # the counts report the need; the guard behind the capacity survives
        assert np.array_equal(got["chain_off"], want["chain_off"])
        cut = dict(want, chains=want["chains"][:len(got["chains"])], seeds=want["seeds"][:len(got["seeds"])])
        K.same(got, cut)
    for kw in (dict(chain_cap=nc - 1), dict(seed_cap=ns - 1)):
        with pytest.raises(N.GbxError) as e:
            host(j, **kw)
        assert e.value.code == N.GBX_ERR_ARG and str(nc) in str(e.value) and str(ns) in str(e.value)
    big = K.synthetic(40, 22, many=(3,))             # more chains and seeds than chain_host's first guess: it regrows
    K.same(host(big), K.reference(big))


def test_determinism_and_half_batches():
    j = K.synthetic(120, 31, many=(7,))
    a, b = device(j)[0], device(j)[0]
    for k in a:
        assert a[k].tobytes() == b[k].tobytes()
    h1, h2 = host(j), host(j)
    for k in h1:
        assert h1[k].tobytes() == h2[k].tobytes() == a[k].tobytes()
    # the same reads as two calls of 60
    def part(lo, hi):
        s0, s1 = int(j["smem_off"][lo]), int(j["smem_off"][hi])
        p0, p1 = int(j["pos_off"][s0]), int(j["pos_off"][s1])
        return dict(j, m=j["m"][s0:s1], n=j["n"][s0:s1], s=j["s"][s0:s1], smem_off=j["smem_off"][lo:hi + 1] - s0, pos=j["pos"][p0:p1],
                    pos_off=j["pos_off"][s0:s1 + 1] - p0, read_off=j["read_off"][lo:hi], read_len=j["read_len"][lo:hi])
    x, y = device(part(0, 60))[0], device(part(60, 120))[0]
    yc = y["chains"].copy()
    yc["read"] += 60
    yc["seed_off"] += len(x["seeds"])
    assert np.concatenate([x["chains"], yc]).tobytes() == a["chains"].tobytes()
    assert np.concatenate([x["seeds"], y["seeds"]]).tobytes() == a["seeds"].tobytes()
    assert np.array_equal(np.concatenate([x["chain_off"], y["chain_off"][1:] + x["chain_off"][-1]]), a["chain_off"])
    assert np.array_equal(np.concatenate([x["l_rep"], y["l_rep"]]), a["l_rep"])


def test_four_host_threads():
    jobs = [K.synthetic(80, 40 + t, many=(t,)) for t in range(4)]
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
