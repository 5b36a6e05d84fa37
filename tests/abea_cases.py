"""Seeded abea read sets that sit on the edges of csrc/abea_kernels.hip: band-variant hand-over, trace-block and
traceback-ring boundaries, wavefront reuse, the plain-division path, the max_gap rule, score ties, odd bytes, the
`fits` refusal.  Builders only: no GPU, no oracle call.  tests/test_abea_edges_cpu.py asserts on the oracle alone that
each set is what it claims to be; tests/test_abea_edges_gpu.py repeats those conditions and compares the kernel.

Every read that is meant for the oracle keeps n_kmers <= n_events + 1: the reference's pair array holds 2 * n_events
entries and a walk is at most n_events + n_kmers - 1 long (align.c:409-500), so only such reads cannot overrun it."""
import numpy as np

from genomicsbench_amd.abea import AbeaReadSet, KMER, make_model
from test_abea_cpu import one_read

BW = 100                                                     # GBX_ABEA_BANDWIDTH


def base_model(seed=4):
    rng = np.random.default_rng(seed)
    return make_model(rng.uniform(65, 125, 4096).astype(np.float32), rng.uniform(1.2, 3.2, 4096).astype(np.float32))


def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(list(alphabet), n))


def oracle_safe(rs):
    """n_kmers <= n_events + 1 for every read (see the module docstring)."""
    n_kmers = rs.seq_len.astype(np.int64) - KMER + 1
    return bool(np.all(n_kmers >= 1) and np.all(n_kmers <= rs.n_events + 1))


def concat(sets, model=None, check=True):
    """Single-read sets (as one_read makes them, all on one model) -> one read set, reads and events back to back."""
    seq_off, ev_off, arena, ev = [], [0], [], []
    pos = 0
    for rs in sets:
        seq_off.append(pos); arena.append(rs.seq_arena); pos += len(rs.seq_arena)
        ev.append(rs.event_mean); ev_off.append(ev_off[-1] + len(rs.event_mean))
    out = AbeaReadSet(seq_off, [s.seq_len[0] for s in sets], np.concatenate(arena), ev_off, np.concatenate(ev),
                      [s.scale[0] for s in sets], [s.shift[0] for s in sets], sets[0].model if model is None else model)
    assert not check or oracle_safe(out)
    return out


def drop_events(rs, keep):
    """The single read `rs` with only the events where `keep` is set."""
    ev = rs.event_mean[keep]
    return AbeaReadSet([0], rs.seq_len, rs.seq_arena, [0, len(ev)], ev, rs.scale, rs.shift, rs.model)


def mid_range(x):
    """abea_kernels.hip's mid_range: 0, or a float whose magnitude lies in [2^-40, 2^40] (NaN and inf are outside)."""
    m = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0x7fffffff)
    return (m == 0) | ((m >= np.uint32((127 - 40) << 23)) & (m <= np.uint32((127 + 40) << 23)))


def is_subnormal(x):
    m = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0x7fffffff)
    return (m != 0) & (m < np.uint32(1 << 23))


def read_ranks(rs, r):
    """k-mer ranks of read r as the kernel ranks them: a byte outside ACGT counts as A (align.c:10-38)."""
    code = np.zeros(256, dtype=np.int64)
    code[ord("C")], code[ord("G")], code[ord("T")] = 1, 2, 3
    c = code[rs.seq_arena[int(rs.seq_off[r]):int(rs.seq_off[r]) + int(rs.seq_len[r])]]
    n = len(c) - KMER + 1
    return sum(c[i:i + n] << (2 * (KMER - 1 - i)) for i in range(KMER))


def takes_fast_division(rs, r):
    """The kernel's per-read choice: every event, scaled mean and stdv of the read in mid_range, every stdv > 0."""
    k = read_ranks(rs, r)
    gm = (rs.scale[r] * rs.model["level_mean"][k]).astype(np.float32) + rs.shift[r]
    gs = rs.model["level_stdv"][k]
    ev = rs.event_mean[int(rs.event_off[r]):int(rs.event_off[r + 1])]
    return bool(mid_range(gm).all() and mid_range(gs).all() and (gs > 0).all() and mid_range(ev).all())


def longest_skip_run(pairs):
    """Longest run of FROM_L moves of a walk: consecutive pairs on one event whose k-mer advances (align.c:466-470)."""
    skip = (np.diff(pairs["read_pos"]) == 0) & (np.diff(pairs["ref_pos"]) == 1)
    best = run = 0
    for s in skip:
        run = run + 1 if s else 0
        best = max(best, run)
    return best


# ---- 1. shape grid --------------------------------------------------------------------------------------------------
GRID_KMERS = [1, 2, 3, 4, 7, 15, 16, 17, 48, 49, 50, 51, 52, 98, 99, 100, 101, 102, 103, 127, 128, 129, 150, 201]
GRID_KMERS_8 = [1, 2, 3, 4, 50, 99, 100, 101, 150]          # 8 events per k-mer: the lengths the oracle accepts


def shape_grid():
    """Single reads around the FAST/general hand-over (n_kmers, n_events near BW / 2, BW - 1, BW, BW + 1), the ring block
    (16 bands) and the traceback ring (4 blocks); then sixteen consecutive lengths at 2 events per k-mer, which take
    n_bands through every residue mod 16 and the block count through every residue mod 4 whatever the grid above gives."""
    model = base_model()
    rng = np.random.default_rng(11)
    sets = []
    for stays in (1, 2, 3, 8):
        for nk in (GRID_KMERS_8 if stays == 8 else GRID_KMERS):
            for noise in (0.0, 0.3):
                rs, _ = one_read(rand_seq(rng, nk + KMER - 1), levels_noise=noise, stays=stays, seed=len(sets), scale=1.02, shift=-1.5, model=model)
                sets.append(rs)
    for nk in range(104, 120):                               # n_bands = 3 n_kmers + 2: sixteen residues mod 16, blocks 20..23
        rs, _ = one_read(rand_seq(rng, nk + KMER - 1), levels_noise=0.3, stays=2, seed=1000 + nk, scale=1.02, shift=-1.5, model=model)
        sets.append(rs)
    return concat(sets)


# ---- 2. many reads per wavefront ------------------------------------------------------------------------------------
def many_reads(n_tiny=6000, n_long=300):
    """n_long reads of 150-300 k-mers (long enough for FAST bands) and n_tiny reads of 1-40 k-mers, 1-3 events each."""
    model = base_model()
    rng = np.random.default_rng(21)
    sets = []
    for i in range(n_long + n_tiny):
        nk = int(rng.integers(150, 301)) if i < n_long else int(rng.integers(1, 41))
        rs, _ = one_read(rand_seq(rng, nk + KMER - 1), levels_noise=0.2, stays=int(rng.integers(1, 4)), seed=i, scale=1.02, shift=-1.5, model=model)
        sets.append(rs)
    order = rng.permutation(len(sets))                       # long and tiny reads mixed in the caller's order
    return concat([sets[i] for i in order])


# ---- 3. the plain-division path -------------------------------------------------------------------------------------
WILD = [1e-30, 3e13, np.inf, -np.inf, np.nan, 1e-40]


def wild_end_events():
    """260-base reads, 2 events per k-mer, one wild value as the first or the last event (the DP trims it), a tame read
    in front of, between and behind them.  -> (read set, indices of the wild reads)"""
    model = base_model()
    rng = np.random.default_rng(31)
    sets, wild = [], []
    for i, (v, at) in enumerate([(v, at) for at in (0, -1) for v in WILD]):
        tame, _ = one_read(rand_seq(rng, 260), levels_noise=0.2, stays=2, seed=100 + i, model=model)
        rs, _ = one_read(rand_seq(rng, 260), levels_noise=0.2, stays=2, seed=200 + i, model=model)
        rs.event_mean[at] = np.float32(v)
        wild.append(len(sets) + 1)
        sets += [tame, rs]
    sets.append(one_read(rand_seq(rng, 260), levels_noise=0.2, stays=2, seed=300, model=model)[0])
    return concat(sets), wild


def scaled_model_reads(factor):
    """The model entries of the k-mers over {G, T} scaled by `factor` (means and stdv; the cached log follows), reads over
    {G, T} on those entries between tame reads over {A, C}.  -> (read set, indices of the scaled reads)"""
    m = base_model()
    rank = np.arange(4096)
    gt = np.all([((rank >> (2 * i)) & 3) >= 2 for i in range(KMER)], axis=0)
    mean, stdv = m["level_mean"].astype(np.float64), m["level_stdv"].astype(np.float64)
    mean[gt] *= factor; stdv[gt] *= factor
    model = make_model(mean.astype(np.float32), stdv.astype(np.float32))
    rng = np.random.default_rng(41)
    sets, scaled = [], []
    for i, (n, stays) in enumerate([(300, 2), (120, 1), (200, 3)]):
        sets.append(one_read(rand_seq(rng, 250, "AC"), levels_noise=0.2, stays=2, seed=400 + i, model=model)[0])
        scaled.append(len(sets))
        sets.append(one_read(rand_seq(rng, n, "GT"), levels_noise=0.2, stays=stays, seed=500 + i, model=model)[0])
    sets.append(one_read(rand_seq(rng, 250, "AC"), levels_noise=0.2, stays=2, seed=403, model=model)[0])
    return concat(sets), scaled


SUBNORMAL_FACTOR = 9e-41                                     # 125 * 9e-41 < 2^-126 = 1.18e-38: means, events and stdv subnormal


def zero_stdv_reads():
    """Four reads; the k-mer in the middle of read 1 has stdv 0 (and log stdv -inf) in the model, and occurs nowhere else.
    -> (read set, 1)"""
    m = base_model()
    rng = np.random.default_rng(51)
    seqs = [rand_seq(rng, n) for n in (200, 300, 180, 260)]
    code = {"A": 0, "C": 1, "G": 2, "T": 3}
    rank = lambda s: sum(code[c] << (2 * (KMER - 1 - i)) for i, c in enumerate(s))
    z = rank(seqs[1][150:150 + KMER])
    hits = sum(rank(s[k:k + KMER]) == z for s in seqs for k in range(len(s) - KMER + 1))
    assert hits == 1
    stdv = m["level_stdv"].copy()
    stdv[z] = 0.0
    with np.errstate(divide="ignore"):
        model = make_model(m["level_mean"], stdv)
    base = base_model()                                      # the events come from the unmodified model
    sets = [one_read(s, levels_noise=0.2, stays=2, seed=600 + i, model=base)[0] for i, s in enumerate(seqs)]
    return concat(sets, model=model), 1


# ---- 4. max_gap -----------------------------------------------------------------------------------------------------
def gap_read(G, n_kmers=1500, at=700):
    """A read whose k-mers [at, at + G) have no events and a model level (400 +- 40) that no event comes near, every
    other k-mer two events at its exact level: the walk skips exactly those G k-mers in one run."""
    rng = np.random.default_rng(61)
    seq = rand_seq(rng, n_kmers + KMER - 1)
    m = base_model()
    probe, ranks = one_read(seq, model=m)
    mean, stdv = m["level_mean"].copy(), m["level_stdv"].copy()
    block = np.array(ranks[at:at + G], dtype=np.int64)
    mean[block], stdv[block] = 400.0, 40.0
    model = make_model(mean, stdv)
    rs, _ = one_read(seq, stays=2, model=model)
    keep = np.ones(2 * n_kmers, dtype=bool)
    keep[2 * at:2 * (at + G)] = False
    rs = drop_events(rs, keep)
    assert oracle_safe(rs)
    return rs


# ---- 5. ties and odd bytes ------------------------------------------------------------------------------------------
def tie_reads(plain=False):
    """Noise-free homopolymer and short-period reads: equal scores wherever two paths see the same levels.  plain: the
    first event of every read is +inf (trimmed by the DP), which puts the read on the kernel's plain-division variant."""
    model = base_model()
    sets = [one_read(seq, stays=stays, model=model)[0] for seq, stays in
            [("A" * 120, 1), ("A" * 120, 2), ("AC" * 80, 2 if plain else 1), ("ACG" * 50, 2), ("T" * 30, 3)]]
    if plain:                                                # (AC x 80 at one event per k-mer is rejected once its first event is gone)
        for rs in sets:
            rs.event_mean[0] = np.float32(np.inf)
    return concat(sets)


def odd_byte_reads():
    """Read 1 holds the bytes 0x00, 0xFF, lowercase c, g, t and N where its events were made for A; reads 0 and 2 are plain."""
    model = base_model()
    rng = np.random.default_rng(71)
    seqs = [rand_seq(rng, 200), rand_seq(rng, 300), rand_seq(rng, 150)]
    odd = [0x00, 0xFF, ord("c"), ord("g"), ord("t"), ord("N")]
    s = list(seqs[1])
    at = list(range(20, 290, 9))
    for p in at:
        s[p] = "A"
    seqs[1] = "".join(s)
    rs = concat([one_read(q, levels_noise=0.2, stays=2, seed=700 + i, model=model)[0] for i, q in enumerate(seqs)])
    for j, p in enumerate(at):
        rs.seq_arena[int(rs.seq_off[1]) + p] = odd[j % len(odd)]
    return rs


def short_last_read(n_bases):
    """An ordinary read, then a read of n_bases bases that ends the arena."""
    model = base_model()
    rng = np.random.default_rng(81 + n_bases)
    return concat([one_read(rand_seq(rng, 150), levels_noise=0.2, stays=2, seed=800, model=model)[0],
                   one_read(rand_seq(rng, n_bases), levels_noise=0.1, stays=2, seed=801, model=model)[0]])


# ---- 6. the refusal -------------------------------------------------------------------------------------------------
def refusal_reads():
    """-> (set with a read of 40 k-mers and 3 events between two ordinary reads, the same set without it, its index,
    that read alone).  A spanned walk of that read needs 40 pairs and its output area holds 6: not for the oracle, unless
    alone and with room.  The read is a homopolymer with exact levels, so every pair of its walk has a perfect emission
    and its 37 skips stay under the gap rule: the size of the walk is the only thing wrong with it."""
    model = base_model()
    rng = np.random.default_rng(91)
    a = one_read(rand_seq(rng, 220), levels_noise=0.2, stays=2, seed=900, model=model)[0]
    b = one_read(rand_seq(rng, 170), levels_noise=0.2, stays=1, seed=901, model=model)[0]
    x = one_read("A" * (40 + KMER - 1), stays=1, seed=902, model=model)[0]
    x = drop_events(x, np.arange(40) < 3)
    return concat([a, x, b], check=False), concat([a, b]), 1, x


# ---- the conditions under which a comparison with the oracle says something: from the oracle's output alone ----------
def accepted(want, reads=None):
    n = want[1] if reads is None else want[1][list(reads)]
    return bool((n > 0).all())


def check_shape_grid(rs, want):
    assert accepted(want), "the oracle rejects grid reads %s" % np.nonzero(want[1] == 0)[0]
    nb = rs.n_bands
    assert set((nb % 16).tolist()) == set(range(16))                       # the partial last flush, tmp_top
    assert set((((nb + 15) // 16) % 4).tolist()) == set(range(4))          # the traceback ring slot the walk ends in
    n_kmers = rs.seq_len.astype(np.int64) - KMER + 1
    for v in (BW // 2, BW - 1, BW, BW + 1):
        assert v in n_kmers and v in rs.n_events


def check_many_reads(rs, want):
    assert accepted(want), "the oracle rejects reads %s" % np.nonzero(want[1] == 0)[0]
    n_kmers = rs.seq_len.astype(np.int64) - KMER + 1
    assert (n_kmers >= 150).sum() >= 300 and (n_kmers <= 40).sum() >= 6000


def check_plain_division(rs, want, odd):
    """the reads `odd` are outside the fast range and accepted; every other read is inside it and accepted"""
    for r in range(rs.n_reads):
        assert takes_fast_division(rs, r) == (r not in odd), r
        assert want[1][r] > 0, "the oracle rejects read %d" % r


def check_subnormal(rs, reads):
    for r in reads:
        k = read_ranks(rs, r)
        assert is_subnormal(rs.event_mean[int(rs.event_off[r]):int(rs.event_off[r + 1])]).all()
        assert is_subnormal(rs.model["level_mean"][k]).all() and is_subnormal(rs.model["level_stdv"][k]).all()


def check_refused_only_for_its_size(alone, want):
    """`want`: the oracle on the read alone, with a pair array that has room for its walk.  Given the room it accepts the
    read - emission, gap and span rules pass - with more pairs than the 2 x events the reference's array holds."""
    assert want[1][0] >= alone.seq_len[0] - KMER + 1 > 2 * alone.n_events[0]
    assert want[1][0] <= 64


def check_gap(rs50, want50, want51):
    assert want50[1][0] > 0 and longest_skip_run(rs50.split_pairs(*want50[:2])[0]) == 50
    assert want51[1][0] == 0
