"""GPU parity of abea_kernel (csrc/abea_kernels.hip) at its own boundaries, on the read sets of tests/abea_cases.py.
Every comparison goes through DeviceAbeaReadSet and is bit-exact against oracle/abea_oracle.c: n_pairs, every pair, and
the count of filled cells (the one observable that pins which bands took the interior variant).  Each test first
repeats, from the oracle's output, the condition under which its comparison says something
(tests/test_abea_edges_cpu.py asserts the same on the CPU)."""
import functools

import numpy as np
import pytest

import abea_cases as AC
from conftest import has_gpu
from genomicsbench_amd.abea import DeviceAbeaReadSet
from oracle import oracle_py as O
from test_abea_gpu import assert_same

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]


def on_device(rs, exact_arenas=False):
    """-> the set after one run on cuda:0.  exact_arenas: the bases and events as tensors of exactly their size, without
    the padding DeviceAbeaReadSet puts behind them."""
    import torch
    dev = torch.device("cuda:0")
    if exact_arenas:
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        d = DeviceAbeaReadSet.from_tensors(dict(seq_off=t(rs.seq_off), seq_len=t(rs.seq_len), seq_arena=t(rs.seq_arena), event_off=t(rs.event_off),
                                                event_mean=t(rs.event_mean), scale=t(rs.scale), shift=t(rs.shift), model=t(rs.model.view(np.uint8))), dev)
    else:
        d = DeviceAbeaReadSet(rs, dev)
    d.run(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d


def compare(rs, d, want):
    import torch
    wo, wn, cells = want
    assert_same(rs, d.results(), (wo, wn))
    got = d.cells(torch.cuda.current_stream().cuda_stream)
    assert got == cells, "filled cells: got %d want %d" % (got, cells)


@functools.lru_cache(maxsize=None)
def gap_case(G):
    rs = AC.gap_read(G)
    return rs, O.abea_oracle(rs, 1, True)


def test_shape_grid():
    """n_kmers and n_events around BW / 2, BW - 1, BW, BW + 1, every n_bands mod 16 and block count mod 4.  Guards the
    FAST bound `m = min(n_kmers - BW - 1 - k_b, n_events - 1 - e_b, ...)` and `b <= n_kmers + 1` (a band taken for interior
    one too early counts BW cells where fewer are filled, and fills cells outside the matrix), the partial last
    `flush`, `tmp_top`, and the four-slot ring of the traceback (`walk_block(ring0) && ... ring3`)."""
    rs = AC.shape_grid()
    want = O.abea_oracle(rs, 8, True)
    AC.check_shape_grid(rs, want)
    compare(rs, on_device(rs), want)


def test_many_reads_per_wavefront_and_a_second_run():
    """More reads than the grid has wavefronts: every wavefront loops for further reads (`for (;;)` with the carried
    `fills`, the `tring` rows and ring registers of the read before), and the cursor passes all three `prio_cut` marks.
    Run twice on one DeviceAbeaReadSet: guards the `hipMemsetAsync(d_work, 0, 256)` of cursor and cell counter - without
    it the second run aligns nothing and the cells double."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rs = AC.many_reads(max(6000, 16 * cus + 64))
    assert rs.n_reads > 16 * cus and rs.n_reads > 12 * cus         # grid <= 16 wavefronts per CU; prio_cut = 4 per CU, tiers end at 12
    want = O.abea_oracle(rs, 8, True)
    AC.check_many_reads(rs, want)
    d = on_device(rs)
    compare(rs, d, want)
    d.out.zero_(); d.n_pairs.zero_()
    d.run(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    compare(rs, d, want)


def test_wild_first_and_last_events_take_plain_division():
    """One event of 1e-30, 3e13, +-inf, NaN or 1e-40 at the start or the end of a read, which the DP trims: the read is
    outside mid_range, so `fdiv` is false and it runs `run_bands(std::false_type{})` - the IEEE division and the
    NaN-aware `score_u > max_score ? ...` selection - and is still aligned (509 pairs).  Tame reads in between keep the
    reciprocal path: guards the per-read `tame` / ballot."""
    rs, wild = AC.wild_end_events()
    want = O.abea_oracle(rs, 8, True)
    AC.check_plain_division(rs, want, wild)
    compare(rs, on_device(rs), want)


@pytest.mark.parametrize("factor", [1e-15, AC.SUBNORMAL_FACTOR], ids=["1e-15", "subnormal"])
def test_scaled_models_take_plain_division(factor):
    """Model means and stdv (and so the events) of some reads scaled by 1e-15, and into the subnormal floats: accepted
    reads whose every division needs the rescaling that the hoisted reciprocal `kr` leaves out.  Guards
    `tame = ... mid_range(gm) && mid_range(gs)` and the `(ev - km) / ks` branch, denormal inputs included."""
    rs, scaled = AC.scaled_model_reads(factor)
    want = O.abea_oracle(rs, 8, True)
    AC.check_plain_division(rs, want, scaled)
    if factor == AC.SUBNORMAL_FACTOR:
        AC.check_subnormal(rs, scaled)
    compare(rs, on_device(rs), want)


def test_zero_stdv_kmer_is_rejected():
    """A k-mer with stdv 0 in the middle of a read.  The oracle rejects the read, so for it this compares the verdict
    (n_pairs == 0) and the filled cells only; its neighbours are compared pair by pair.  Guards `gs > 0.f` in `tame`."""
    rs, z = AC.zero_stdv_reads()
    want = O.abea_oracle(rs, 4, True)
    assert want[1][z] == 0 and AC.accepted(want, [r for r in range(rs.n_reads) if r != z])
    assert not AC.takes_fast_division(rs, z)
    compare(rs, on_device(rs), want)


@pytest.mark.parametrize("G", [50, 51])
def test_max_gap(G):
    """A run of exactly 50 skipped k-mers is kept, one of 51 rejected (align.c:534, `max_gap > 50`).  Guards the
    branch-free `curr_gap = (curr_gap + 1) & -(int)(from >> 1)` and `!(max_gap > 50)`.  (1 500 k-mers, 4 400 bands.)"""
    AC.check_gap(gap_case(50)[0], gap_case(50)[1], gap_case(51)[1])
    rs, want = gap_case(G)
    compare(rs, on_device(rs), want)


@pytest.mark.parametrize("plain", [False, True], ids=["reciprocal", "plain"])
def test_ties(plain):
    """Noise-free homopolymer and short-period reads: equal candidate scores and equal band corners all along.  Guards
    the order D < U < L of `f = max_score == score_u ? 1 : f; ... == score_l ? 2 : f` - the `fmaxf` form of tame reads,
    and with a trimmed +inf first event the `score_u > max_score ? ...` form of the plain-division variant - and the
    strict `lli < uri` of the band placement."""
    rs = AC.tie_reads(plain)
    want = O.abea_oracle(rs, 2, True)
    assert AC.accepted(want)
    assert [AC.takes_fast_division(rs, r) for r in range(rs.n_reads)] == [not plain] * rs.n_reads
    compare(rs, on_device(rs), want)


def test_odd_bytes():
    """0x00, 0xFF, lowercase and N among the bases rank as A (`base_rank`, the 8-byte `kmer_bytes` load and its shifts)."""
    rs = AC.odd_byte_reads()
    want = O.abea_oracle(rs, 2, True)
    assert AC.accepted(want)
    compare(rs, on_device(rs), want)


@pytest.mark.parametrize("n_bases", [6, 7, 8, 9])
def test_short_read_ends_the_arena(n_bases):
    """The last read of an arena with nothing behind it, 1 to 4 k-mers long: `kmer_bytes` takes the byte-wise branch
    (`k + 8 <= slen` fails) for all, some, or none of its k-mers; `eload` / `kload` clamp every look-ahead index."""
    rs = AC.short_last_read(n_bases)
    want = O.abea_oracle(rs, 1, True)
    assert AC.accepted(want) and rs.seq_off[1] + n_bases == len(rs.seq_arena)
    compare(rs, on_device(rs, exact_arenas=True), want)


def test_walk_longer_than_the_output_area_is_refused():
    """40 k-mers on 3 events: a spanned walk has at least 40 pairs, the read's output area holds 2 * 3, so the expected
    result is n_pairs == 0 with the area untouched - by derivation, the oracle is not run on this read (it would
    overrun).  Its neighbours equal the oracle on the set without it.  The read is a noise-free homopolymer: the oracle,
    run on it alone with room for the walk, accepts it, so its size is all that refuses it.  Guards
    `fits = n_out <= cap`, `fits` in `ok`, and `if (fits)` in front of the pair store.  Cells: a 3 x 40 matrix lies
    inside every band that crosses it, so all 120 are filled."""
    import torch
    with_x, without, x, alone = AC.refusal_reads()
    wo, wn, cells = O.abea_oracle(without, 2, True)
    assert AC.accepted((wo, wn))
    AC.check_refused_only_for_its_size(alone, O.abea_oracle(alone, 1, room=64))
    d = on_device(with_x)
    go, gn = d.results()
    assert gn[x] == 0
    a, b = 2 * int(with_x.event_off[x]), 2 * int(with_x.event_off[x + 1])
    assert b - a == 6 and not go[a:b].view(np.int32).any(), "pairs written for the refused read: %s" % go[a:b]
    keep = [r for r in range(with_x.n_reads) if r != x]
    assert np.array_equal(gn[keep], wn)
    for g, w in zip([p for r, p in enumerate(with_x.split_pairs(go, gn)) if r != x], without.split_pairs(wo, wn)):
        assert np.array_equal(g, w)
    assert d.cells(torch.cuda.current_stream().cuda_stream) == cells + 3 * 40
