"""The CIGAR stage on the GPU (gbx_mem_cigar_device / gbx_mem_cigar_host), byte-exact against the restated rules of
tests/mem_cigar_ref.py on the gbx_mem_aln records, the CIGAR words and their count.  The kernel has one layout and one code
path for every region length, so there is no size switch to straddle; the strip edges (|Q| around 64 and 128) and a band wider
than a strip are the places where it changes gear."""
import ctypes as C
import threading

import numpy as np
import pytest

from genomicsbench_amd import _native as N
from genomicsbench_amd import bsw_seeds as BS
from genomicsbench_amd import fmi as FM
from genomicsbench_amd import mem_chain as MC
from genomicsbench_amd import mem_cigar as MG
import mem_cigar_cases as K
import mem_cigar_ref as R

pytestmark = pytest.mark.gpu
GUARD = 0x5a5a5a5a


def params_of(j):
    return MG.make_params(**j["params"])


def host(j, **kw):
    return MG.cigar_host(params_of(j), j["seeds"], j["res"], j["text"], j["qer"], j["L"], j["contig_off"], **kw)


def worst_rooms(j):
    """gbx_mem_cigar_record_z_bytes of every record that has a region (an upper bound of the room it is given)."""
    p = params_of(j)
    res = np.ascontiguousarray(j["res"]).view(R.RESULT_DTYPE).reshape(-1)
    return [int(MG.lib().gbx_mem_cigar_record_z_bytes(C.byref(p), int(r["qe"] - r["qb"]), int(r["re"] - r["rb"]))) if r["qb"] >= 0 else 0
            for r in res]


def device(j, cigar_cap=None, z_bytes=None, slack=5):
    """gbx_mem_cigar_device on the job's arrays with `slack` records of all -1 behind them (n is a capacity, not a count) and 16
    guard words behind cigar_cap.  -> ((alns, cigar cut to the capacity), n_cigar, guards intact)."""
    import torch
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    n = len(j["seeds"]) + slack
    seeds = np.concatenate([j["seeds"], np.zeros(slack, R.SEED_DTYPE)])
    res = np.concatenate([j["res"], np.full((slack, 8), -1, np.int32)])
    d_seeds, d_res = t(seeds.view(np.uint8)), t(res)
    d_text, d_qer, d_co = t(j["text"]), t(j["qer"]), t(j["contig_off"])
    want_words = 4 * n + 64 if cigar_cap is None else cigar_cap
    d_alns = torch.zeros(n * 48, dtype=torch.uint8, device=dev)
    d_cigar = torch.from_numpy(np.full(want_words + 16, GUARD, np.uint32).view(np.int32)).to(dev)
    d_n = torch.zeros(1, dtype=torch.int64, device=dev)
    zb = sum(worst_rooms(j)) if z_bytes is None else z_bytes
    wb = MG.lib().gbx_mem_cigar_workspace_bytes(n, zb)
    d_w = torch.empty(max(wb, 1), dtype=torch.uint8, device=dev)
    p = params_of(j)
    N.check(MG.lib().gbx_mem_cigar_device(C.byref(p), n, d_seeds.data_ptr(), d_res.data_ptr(), d_text.data_ptr(), len(j["text"]),
                                          d_qer.data_ptr(), len(j["qer"]), int(j["L"]), len(j["contig_off"]) - 1, d_co.data_ptr(),
                                          d_alns.data_ptr(), d_cigar.data_ptr(), want_words, d_n.data_ptr(), d_w.data_ptr(), wb, None))
    torch.cuda.synchronize()
    nc = int(d_n.cpu().numpy()[0])
    alns = d_alns.cpu().numpy().view(MG.ALN_DTYPE)
    cg = d_cigar.cpu().numpy().view(np.uint32)
    intact = bool((cg[want_words:] == GUARD).all())
    tail = alns[len(j["seeds"]):]
    tail_ok = bool((tail["rid"] == -1).all() and (tail["n_cigar"] == 0).all() and (tail["cigar_off"] == nc).all())
    return (alns[:len(j["seeds"])].copy(), cg[:min(nc, want_words)].copy()), nc, intact and tail_ok


def both_entries(j, want=None):
    want = want or K.reference(j)
    got, nc, ok = device(j)
    assert ok and nc == len(want[1])
    K.same(got, want)
    K.same(host(j), want)
    return want


@pytest.mark.parametrize("name", sorted(K.hand_built()))
def test_hand_built_cases(name):
    """simple: no-DP path, mismatch, inserted / deleted base, N, 1 x 1.  strand: homopolymer indels and clips on both strands,
    rb < L < re, all -1.  squeeze: leading / trailing deletion.  ties: m == e, h == f, e == t, f == t.  tries*: the band doubles,
    score == last, the stop at 4 w, w2 capped by r.w.  band_and_strips: 2 w + 1 < |Q|, |Q| of 63 .. 129, a band wider than a
    strip.  scoring: a = 2 and unequal gap costs."""
    j = K.hand_built()[name]
    want = both_entries(j)
    K.check_invariants(j, *want)
    if name == "band_and_strips":
        for lq in (63, 64, 65, 127, 128, 129):
            for kind in ("ins", "del", "sub"):
                assert "q%d_%s" % (lq, kind) in j["names"]


def read_pairs(g, n, seed):
    """n reads of 101 .. 151 bases cut from g, both strands, with substitutions and short indels."""
    rng = np.random.default_rng(seed)
    reads = []
    for _ in range(n):
        ln = int(rng.integers(101, 152))
        at = int(rng.integers(0, len(g) - ln - 8))
        piece = g[at:at + ln + 8]
        subs = set(int(x) for x in rng.integers(0, ln, int(rng.integers(0, 4))))
        ins = set(int(x) for x in rng.integers(30, ln - 30, 1)) if rng.random() < 0.3 else set()
        dele = set(int(x) for x in rng.integers(30, ln - 30, int(rng.integers(1, 3)))) if rng.random() < 0.3 else set()
        rd = K.mutate(piece, subs, ins, dele)[:ln]
        reads.append(K.revcomp(rd) if rng.random() < 0.5 else rd)
    lens = np.array([len(r) for r in reads], dtype=np.int32)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    return FM.FmiReadSet(np.concatenate(reads).astype(np.uint8), offs, lens)


def test_whole_pipeline_on_one_stream():
    """smem -> sal -> chain -> extend -> cigar queued back to back on one stream, n = seed_cap, one synchronise at the end; the
    CIGAR stage is compared with the reference run on the extension's downloaded results."""
    import torch
    from genomicsbench_amd.datagen import gen_fmi_genome
    g = gen_fmi_genome(50_000, 7301)
    co = np.array([0, 21_000, 50_000], dtype=np.int64)
    rs = read_pairs(g, 200, 7302)
    idx, smp = FM.build_index(g, sa_compx=3)
    text = MC.text_of(g)
    sp = BS.make_seed_params()
    cap = 6000
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
        p = MG.make_params()
        z_bytes = 2500 * MG.lib().gbx_mem_cigar_record_z_bytes(C.byref(p), 151, 200)
        cg = MG.DeviceMemCigar(ext, p, cigar_cap=8 * cap, z_bytes=z_bytes)
        assert cg.n == mc.seed_cap == cap
        cg.run(s.cuda_stream)
    s.synchronize()
    chains = mc.results()
    n_seeds = len(chains["seeds"])
    assert 200 <= n_seeds < cap
    seeds = mc.seeds.cpu().numpy().view(BS.SEED_DTYPE)[:cap]
    res = ext.results()
    assert (res[n_seeds:] == -1).all() and (res[:n_seeds, 2] >= 0).all()
    got = cg.results()
    j = dict(params={}, L=len(g), contig_off=co, text=text, qer=rs.enc, seeds=seeds, res=res)
    want = K.reference_c(j)
    K.same(got, want)
    alns = got[0]
    assert (alns["rid"][:n_seeds] >= 0).all() and (alns["rid"][n_seeds:] == -1).all()
    assert set(alns["is_rev"][:n_seeds].tolist()) == {0, 1} and set(alns["rid"][:n_seeds].tolist()) == {0, 1}
    ops = got[1] & 15
    assert (ops == R.I).any() and (ops == R.D).any() and (ops == R.S).any() and (alns["nm"] > 0).any()
    K.check_invariants(j, *got)


def short_job():
    """Reads so short that a record's room does not depend on its band (d + 3 rules it): gbx_mem_cigar_record_z_bytes exactly."""
    g = K.genome()
    b = K.Builder()
    for c in range(5):
        at = 100 + 40 * c
        b.add("short%d" % c, K.mutate(g[at:at + 18 + c], dele={9}), at, at + 18 + c, rev=bool(c & 1))
    return b.job()


def test_capacity():
    j = K.synthetic(30, 51)
    want = K.reference_c(j)
    nc = len(want[1])
    assert nc > 40
    for cap in (nc - 1, 7, 0, nc):
        got, gc, ok = device(j, cigar_cap=cap)
        assert gc == nc and ok                        # the count reports the need; the guard behind the capacity survives
        assert got[0].tobytes() == want[0].tobytes()  # cigar_off stays true
        assert np.array_equal(got[1], want[1][:cap])
    with pytest.raises(N.GbxError) as e:
        host(j, cigar_cap=nc - 1)
    assert e.value.code == N.GBX_ERR_ARG and str(nc) in str(e.value)
    K.same(host(j, cigar_cap=nc), want)
    big = K.synthetic(8, 52, read_len=(20, 30), a=1, b=1, o_del=1, e_del=1, o_ins=1, e_ins=1)     # more words than cigar_host's first guess
    K.same(host(big), K.reference_c(big))


def test_direction_room_too_small_for_the_last_record_only():
    j = short_job()
    want = K.reference(j)
    rooms = worst_rooms(j)
    assert all(r > 0 for r in rooms) and (want[0]["w"] > 0).all()
    got, nc, ok = device(j, z_bytes=sum(rooms))
    assert ok
    K.same(got, want)
    got, nc, ok = device(j, z_bytes=sum(rooms) - 1)
    last = len(rooms) - 1
    assert ok and nc == len(want[1]) - want[0][last]["n_cigar"]
    assert got[0][last]["rid"] == -2 and got[0][last]["n_cigar"] == 0 and got[0][last]["cigar_off"] == nc
    assert got[0][:last].tobytes() == want[0][:last].tobytes() and np.array_equal(got[1], want[1][:nc])
    got, nc, ok = device(j, z_bytes=0)                # nothing fits: every region comes back -2, nothing is written
    assert ok and nc == 0 and (got[0]["rid"] == -2).all()


def test_determinism():
    j = K.synthetic(60, 61)
    a, b = device(j)[0], device(j)[0]
    h1, h2 = host(j), host(j)
    for x, y, u, v in zip(a, b, h1, h2):
        assert x.tobytes() == y.tobytes() == u.tobytes() == v.tobytes()
    K.same(a, K.reference_c(j))


def test_four_host_threads():
    jobs = [K.synthetic(40, 70 + t) for t in range(4)]
    want = [K.reference_c(j) for j in jobs]
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
