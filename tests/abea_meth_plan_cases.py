"""Hand-made reads for the call-methylation site planner on the device (tests/test_abea_meth_plan_gpu.py) and for the host build of
its rules (tests/test_abea_meth_plan_cpu.py).  A case is one read: its reference segment, its event-alignment record, its strand,
its start and what the planner must make of it -- (first CpG, last CpG, CpGs) per site, relative to the segment.  The CPU test holds
every claim against the host planner.  The reads of a batch lie in one arena with the bytes b"GCG" between them, so that a walk that
leaves its segment finds a CpG that is not there."""
import numpy as np

from genomicsbench_amd.abea import PAIR_DTYPE

PAD = b"GCG"


def ref_with(n, at, fill=b"A"):
    b = bytearray(fill * n)
    for p in at:
        b[p:p + 2] = b"CG"
    return bytes(b)


def linear(n, pos=0, per_base=2):
    return [(pos + p, per_base * p) for p in range(n)]


class Case:
    def __init__(self, name, ref, rec=None, rc=0, pos=0, sites=(), seq_len=None):
        self.name, self.ref, self.rc, self.pos = name, ref, rc, pos
        self.rec = linear(len(ref) + 30, pos) if rec is None else rec
        self.sites, self.seq_len = sites, seq_len     # sites: a list of triples, or a count; seq_len: the sites' L, where the case is about it


def _iupac():
    ref = b"A" * 30 + b"cg" + b"t" * 20 + b"SK" + b"n" * 20 + b"yG" + b"#x!" + b"RWVHDNMB" + b"k" + b"u" * 30
    assert len(ref) == 118
    return ref


def _random_ref(n, seed):
    rng = np.random.default_rng(seed)
    return bytes(np.frombuffer(b"ACGTacgtNRYSK", np.uint8)[rng.integers(0, 13, n)])


def cases():
    one = ref_with(100, [40])
    many = ref_with(30 + 22 * 70 + 30, [30 + 22 * k for k in range(70)])
    gapped = [q for q in linear(130) if not (28 <= q[0] <= 33 or 48 <= q[0] <= 53)]
    return [
        Case("c63", ref_with(200, [63]), sites=[(63, 63, 1)]),                                # the C in one trip of 64, the G in the next
        Case("c127", ref_with(200, [127]), pos=1000, sites=[(127, 127, 1)]),
        Case("g_last", ref_with(100, [98]), sites=[(98, 98, 1)], seq_len=[12]),              # the G is the last base; L clamped to 12
        Case("c_last", ref_with(100, [40])[:-1] + b"C", sites=[(40, 40, 1)]),                # a C at the end, a G behind the segment
        Case("clamped_last", ref_with(100, [50, 95]), sites=[(50, 50, 1), (95, 95, 1)], seq_len=[21, 15]),
        Case("sep10_boundary", ref_with(200, [58, 68]), sites=[(58, 68, 2)]),
        Case("sep11_boundary", ref_with(200, [58, 69]), sites=[(58, 58, 1), (69, 69, 1)]),
        Case("long_group", ref_with(300, range(30, 171, 10)), sites=[(30, 170, 15)]),        # spans more than two trips
        Case("span200", ref_with(300, range(30, 231, 10)), sites=[(30, 230, 21)]),
        Case("span201", ref_with(300, list(range(30, 221, 10)) + [229, 231]), sites=[]),
        Case("first20", ref_with(100, [20]), sites=[]),                                      # sub_start_pos 10
        Case("first21", ref_with(100, [21]), sites=[(21, 21, 1)]),                           # sub_start_pos 11
        Case("cgcgcg", b"A" * 40 + b"CGCGCG" + b"A" * 54, sites=[(40, 44, 3)]),
        Case("cgrun_boundary", b"T" * 60 + b"CGCGCGCG" + b"T" * 60, sites=[(60, 66, 4)]),
        Case("iupac", _iupac(), sites=[(30, 30, 1), (52, 52, 1), (74, 74, 1), (86, 86, 1)]),
        Case("len0", b"", rec=linear(30), sites=[]),
        Case("len1", b"C", rec=linear(30), sites=[]),
        Case("len2", b"CG", rec=linear(30), sites=[]),
        Case("empty_record", one, rec=[], sites=[]),
        Case("one_pair", one, rec=[(40, 5)], sites=[]),
        Case("gapped", one, rec=gapped, sites=[(40, 40, 1)]),                                # both lower bounds land above their targets
        Case("end_past", one, rec=linear(46), sites=[]),                                     # calling_end past the last ref_pos
        Case("start_before", one, rec=linear(130)[35:], sites=[]),                           # calling_start before the first ref_pos
        Case("diff10", one, rec=[(p, p // 2) for p in range(130)], sites=[]),
        Case("diff11", one, rec=[(p, (p * 11) // 20) for p in range(130)], sites=[(40, 40, 1)]),
        Case("reverse", one, rec=[(7000 + p, 500 - 2 * p) for p in range(130)], rc=1, pos=7000, sites=[(40, 40, 1)]),
        Case("many_groups", many, sites=70),                                                 # more than 64 kept groups in one read
        Case("random", _random_ref(1500, 11), sites=None),
        Case("random_reverse", _random_ref(900, 12), rec=[(p, 4000 - 3 * p) for p in range(930)], rc=1, sites=None),
    ]


def batch(cs):
    """-> dict(ref_off, ref_len, ref_arena, ref_start_pos, rc, rec_off, rec) of the cases' reads"""
    arena, ref_off, rec, rec_off = bytearray(PAD), [], [], [0]
    for c in cs:
        ref_off.append(len(arena))
        arena += c.ref + PAD
        rec += c.rec
        rec_off.append(len(rec))
    return dict(ref_off=np.array(ref_off, np.int64), ref_len=np.array([len(c.ref) for c in cs], np.int32), ref_arena=np.frombuffer(bytes(arena), np.uint8),
                ref_start_pos=np.array([c.pos for c in cs], np.int32), rc=np.array([c.rc for c in cs], np.uint8), rec_off=np.array(rec_off, np.int64),
                rec=np.array(rec, PAIR_DTYPE) if rec else np.zeros(0, PAIR_DTYPE))


def edge_batch():
    return batch(cases())


def tiny_batch(n):
    """n tiny reads, every third one without a site: the offsets of the planner's scan at its block edge"""
    with_site, without = Case("tiny", ref_with(60, [30]), sites=[(30, 30, 1)]), Case("tiny_none", b"A" * 40, sites=[])
    return batch([without if r % 3 == 1 else with_site for r in range(n)])


def planner_args(b):
    return (b["ref_off"], b["ref_len"], b["ref_arena"], b["ref_start_pos"], b["rc"], b["rec_off"], b["rec"])
