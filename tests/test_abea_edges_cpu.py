"""abea edge cases on the CPU: the read sets of tests/abea_cases.py are what they claim to be, judged by the oracle
(oracle/abea_oracle.c) alone.  A read the oracle rejects compares as 0 == 0 on the GPU and proves nothing there, so
tests/test_abea_edges_gpu.py rests on these conditions and repeats them before it compares."""
import numpy as np

import abea_cases as AC
from genomicsbench_amd.abea import KMER
from oracle import oracle_py as O


def test_mid_range_restatement():
    x = np.array([0.0, -0.0, 2.0 ** -40, -2.0 ** 40, 2.0 ** -41, np.nextafter(np.float32(2.0 ** 40), np.float32(np.inf)), 1e-30, 3e13,
                  np.inf, -np.inf, np.nan, 1e-40, 100.0], dtype=np.float32)
    assert AC.mid_range(x).tolist() == [True, True, True, True, False, False, False, False, False, False, False, False, True]
    assert AC.is_subnormal(np.array([1e-40, 1.17e-38, 1.18e-38, 0.0], dtype=np.float32)).tolist() == [True, True, False, False]


def test_shape_grid_is_accepted_and_covers_the_block_residues():
    rs = AC.shape_grid()
    want = O.abea_oracle(rs, 8, True)
    AC.check_shape_grid(rs, want)
    assert want[2] > 0


def test_many_reads_are_accepted():
    rs = AC.many_reads()
    assert rs.n_reads == 6300
    AC.check_many_reads(rs, O.abea_oracle(rs, 8, True))


def test_wild_end_events_are_trimmed_not_rejected():
    rs, wild = AC.wild_end_events()
    assert len(wild) == 12
    want = O.abea_oracle(rs, 8, True)
    AC.check_plain_division(rs, want, wild)
    for r in wild:                                           # the wild event is in no pair: 2 * 255 events, one trimmed
        assert want[1][r] == 509


def test_scaled_models_are_accepted_and_subnormal():
    for factor in (1e-15, AC.SUBNORMAL_FACTOR):
        rs, scaled = AC.scaled_model_reads(factor)
        AC.check_plain_division(rs, O.abea_oracle(rs, 8, True), scaled)
    AC.check_subnormal(rs, scaled)


def test_zero_stdv_is_rejected():
    rs, z = AC.zero_stdv_reads()
    want = O.abea_oracle(rs, 4, True)
    assert [AC.takes_fast_division(rs, r) for r in range(rs.n_reads)] == [r != z for r in range(rs.n_reads)]
    assert want[1][z] == 0 and AC.accepted(want, [r for r in range(rs.n_reads) if r != z])


def test_gap_of_50_is_kept_and_51_rejected():
    rs48, rs50, rs51 = AC.gap_read(48), AC.gap_read(50), AC.gap_read(51)
    assert rs51.seq_len[0] == rs50.seq_len[0] and rs51.n_events[0] == rs50.n_events[0] - 2      # one more k-mer without events
    AC.check_gap(rs50, O.abea_oracle(rs50), O.abea_oracle(rs51))
    w = O.abea_oracle(rs48)
    assert w[1][0] > 0 and AC.longest_skip_run(rs48.split_pairs(*w)[0]) == 48


def test_tie_and_odd_byte_reads_are_accepted():
    rs = AC.tie_reads()
    want = O.abea_oracle(rs, 2)
    assert AC.accepted(want)
    p = rs.split_pairs(*want)[0]                              # A x 120, one event per k-mer: every level equal, still the diagonal
    assert len(p) == 115
    rs = AC.tie_reads(plain=True)
    assert AC.accepted(O.abea_oracle(rs, 2)) and not any(AC.takes_fast_division(rs, r) for r in range(rs.n_reads))
    rs = AC.odd_byte_reads()
    assert AC.accepted(O.abea_oracle(rs, 2))
    odd = set(rs.seq_arena[int(rs.seq_off[1]):int(rs.seq_off[2])].tolist()) - set(b"ACGT")
    assert odd == {0x00, 0xFF, ord("c"), ord("g"), ord("t"), ord("N")}
    for n in (6, 7, 8, 9):
        rs = AC.short_last_read(n)
        assert rs.seq_len[1] == n and rs.seq_off[1] + n == len(rs.seq_arena) and AC.accepted(O.abea_oracle(rs, 1))


def test_refusal_set():
    with_x, without, x, alone = AC.refusal_reads()
    n_kmers = with_x.seq_len.astype(np.int64) - KMER + 1
    assert n_kmers[x] == 40 and with_x.n_events[x] == 3 and n_kmers[x] > 2 * with_x.n_events[x]
    assert not AC.oracle_safe(with_x) and AC.oracle_safe(without)
    assert AC.accepted(O.abea_oracle(without, 2))
    AC.check_refused_only_for_its_size(alone, O.abea_oracle(alone, 1, room=64))
    # the neighbours are the same reads in both sets
    assert np.array_equal(np.delete(with_x.seq_len, x), without.seq_len)
    a, b = int(with_x.event_off[x]), int(with_x.event_off[x + 1])
    assert np.array_equal(np.delete(with_x.event_mean, np.arange(a, b)), without.event_mean)
