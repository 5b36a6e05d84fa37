"""GPU parity of csrc/kmer_kernels.hip at its own edges, on the calls of tests/kmer_cases.py: position counts on, before and
behind the count pass's 256-position units at every start residue of its 16-byte words, with hostile bytes around the
reads; bytes above 3; palindromes and reverse-strand-only k-mers; read counts around the unit kernel's 1024 threads with
unit-less reads first, last, in runs and singly; counters on both sides of a lane's, a wavefront's, a round's and a
workgroup's share of the sweeps and of the selection scan's second trip; histogram bins at the clamp; selections cut at
sel_cap inside a lane, at a wavefront's, a round's, a workgroup's and a slice's end; k-mers on both sides of the slice
borders of k = 16 and in slices 0, 7 and 15 of k = 17.  Every comparison is exact against the case's own expectation
(tests/test_kmer_edges_cpu.py asserts, on the CPU alone, that tests/kmer_ref.py counts the same and that each call is what it
is named for): stats, the whole histogram and the selection in order, from gbx_kmer_count_host and gbx_kmer_count_device."""
import ctypes as C

import numpy as np
import pytest

import kmer_cases as KC
from genomicsbench_amd import _native as N
from genomicsbench_amd import kmer as K

pytestmark = pytest.mark.gpu
CASES = {c.name: c for c in KC.all_cases()}
GUARD = 64                               # sentinel entries behind sel_cap in the device entry's outputs
SENT_KMER, SENT_COUNT = -0x0123456789abcdef, 0x5a5a5a5a


def same(got, want, cap, what):
    """got against the first `cap` of the expectation's selection; the stats are those of the whole selection"""
    gs, gh, gk, gc = got
    ws, wh, wk, wc = want
    assert gs == ws, "%s: stats %r, expected %r" % (what, gs, ws)
    assert np.array_equal(gh, wh), "%s: histogram differs in bins %r" % (what, np.flatnonzero(np.asarray(gh) != wh)[:8].tolist())
    assert np.array_equal(gk, wk[:cap]), "%s: selected k-mers %r ..., expected %r ..." % (what, gk[:8].tolist(), wk[:8].tolist())
    assert np.array_equal(gc, wc[:cap]), "%s: selected counts %r ..., expected %r ..." % (what, gc[:8].tolist(), wc[:8].tolist())


def run_host(c):
    """gbx_kmer_count_host itself, so that a sel_cap below the need shows its return code -> (rc, stats, hist, kmers, counts)"""
    r, cap = c.reads, c.sel_cap
    p = K.KmerParams(c.k, c.n_hist, c.min_freq, c.max_freq)
    st = K.KmerStats()
    hist = np.full(max(c.n_hist, 1), -1, dtype=np.int64)
    km, cn = np.zeros(max(cap, 1), dtype=np.uint64), np.zeros(max(cap, 1), dtype=np.uint32)
    rc = N.lib().gbx_kmer_count_host(C.byref(p), r.n_reads, N.ptr(r.enc), r.enc.size, N.ptr(r.read_off), N.ptr(r.read_len), C.byref(st),
                                     N.ptr(hist) if c.n_hist else None, N.ptr(km), N.ptr(cn), cap)
    n = min(int(st.n_selected), cap)
    return rc, ({f: int(getattr(st, f)) for f in K.STATS_FIELDS}, hist[:c.n_hist], km[:n], cn[:n])


def load(d, c):
    """case c on the DeviceKmer d: its reads, its parameters, and outputs with GUARD sentinel entries behind sel_cap"""
    import torch
    r = c.reads
    d.n_reads = r.n_reads
    d.enc, d.read_off, d.read_len = (torch.from_numpy(a).to(d.dev) for a in (r.enc, r.read_off, r.read_len))
    d.set_params(c.k, c.n_hist, c.min_freq, c.max_freq, c.sel_cap)
    d.sel_kmer = torch.full((c.sel_cap + GUARD,), SENT_KMER, dtype=torch.int64, device=d.dev)
    d.sel_count = torch.full((c.sel_cap + GUARD,), SENT_COUNT, dtype=torch.int32, device=d.dev)


def run_device(d, c, what):
    import torch
    d.run()
    torch.cuda.synchronize()
    same(d.results(), c.want(), c.sel_cap, what)
    assert (d.sel_kmer[c.sel_cap:] == SENT_KMER).all().item() and (d.sel_count[c.sel_cap:] == SENT_COUNT).all().item(), \
        "%s: the device entry wrote behind sel_cap = %d" % (what, c.sel_cap)


def new_device(c):
    d = K.DeviceKmer(K.KmerReadSet.from_codes([np.zeros(2, dtype=np.uint8)]), "cuda:0", 1)
    load(d, c)
    return d


@pytest.mark.parametrize("name", list(CASES))
def test_edges(name):
    """Guards, by family: chunk_word - the unit's position count and its [first, end) byte window inside the aligned words,
    whatever lies around the read; high_bits - the & 3 on every base; strands - the rolled reverse code and min(fwd, rev);
    units - the unit kernel's shares and scan and the count pass's binary search past reads without units; sweep - the
    summary's lane, wavefront and workgroup sums, bin 1 in its register, the clamp at n_hist - 1, >= 16; select - the scan's
    carry across trips, the wave scan, the workgroup prefix and the running slot, the early leave and the o < sel_cap guard;
    slices - lo and the running total across slices."""
    c = CASES[name]
    rc, got = run_host(c)
    if c.sel_cap < c.need:
        assert rc == N.GBX_ERR_ARG and got[0]["n_selected"] == c.need and str(c.need) in N.lib().gbx_last_error().decode()
    else:
        assert rc == N.GBX_OK, N.lib().gbx_last_error().decode()
    same(got, c.want(), c.sel_cap, name + " gbx_kmer_count_host")
    run_device(new_device(c), c, name + " gbx_kmer_count_device")


def test_one_workspace_through_k_and_twice():
    """a k = 16 call, a k = 11 call on the same (larger) workspace, the k = 16 call again, and one call twice in a row: what
    a call leaves in the table, in the workgroups' counts and in the running total is not read by the next one"""
    a, b = CASES["slices_k16_gap"], CASES["select_every_64th"]
    d = new_device(a)
    run_device(d, a, "k = 16 first")
    big = d.work
    load(d, b)
    assert d.work is big and d.work_bytes < big.numel()
    run_device(d, b, "k = 11 on the k = 16 workspace")
    run_device(d, b, "k = 11 again")
    load(d, a)
    assert d.work is big
    run_device(d, a, "k = 16 after k = 11")
    cut = CASES["slices_k16_cut_in_1"]
    load(d, cut)
    run_device(d, cut, "k = 16 cut inside slice 1")
    run_device(d, cut, "k = 16 cut inside slice 1, again")
