"""Restatement of index construction for the tests of `mem index` and gbx_fmi_build_* (tests/test_mem_index_cpu.py,
tests/test_mem_index_gpu.py).  It shares no code with the product or with fmi.build_index: a suffix array by sorted() on byte
strings, the BWT, the checkpoints and the samples by plain loops, lrand48 as its 48-bit LCG, and FASTA text to the four reference
files (.ann, .amb, .pac, .0123) as csrc/drivers/ref_files.h documents them.  Parity with bwa-mem2 itself is UNPINNED."""
import struct

MASK48 = (1 << 48) - 1


class Rand48:
    """lrand48 after srand48(seed): X = (0x5DEECE66D X + 0xB) mod 2^48 from X = seed << 16 | 0x330E; a draw is X >> 17."""

    def __init__(self, seed):
        self.x = (seed << 16 | 0x330E) & MASK48

    def next(self):
        self.x = (0x5DEECE66D * self.x + 0xB) & MASK48
        return self.x >> 17


def text_of(genome):
    g = [int(c) for c in genome]
    return g + [3 - c for c in reversed(g)]


def suffix_array(text):
    """Rows of the n + 1 suffixes of text (codes 0..3); the empty suffix sorts first.  sorted() on byte strings: windows of the
    suffixes, the groups that tie on a window sorted again on the next, twice as wide (whole suffixes as keys would take
    n^2 / 2 bytes).  A suffix that ends inside a window has a shorter key than the ones it ties with, and sorts first."""
    b = bytes(int(c) + 1 for c in text)
    out, todo = [], [(list(range(len(b) + 1)), 0, 64)]
    while todo:
        rows, depth, width = todo.pop()
        if len(rows) == 1:
            out.append(rows[0])
            continue
        rows = sorted(rows, key=lambda i: b[i + depth:i + depth + width])
        groups, at = [], 0
        while at < len(rows):
            k = b[rows[at] + depth:rows[at] + depth + width]
            end = at + 1
            while end < len(rows) and b[rows[end] + depth:rows[end] + depth + width] == k:
                end += 1
            groups.append((rows[at:end], depth + width, 2 * width))
            at = end
        todo.extend(reversed(groups))                    # a stack: the first group is finished first
    return out


def build(genome, sa_compx):
    """-> dict(ref_seq_len, count[5], sentinel_index, cp_occ bytes, ms bytes, ls bytes, sa)."""
    text = text_of(genome)
    sa = suffix_array(text)
    n1 = len(sa)
    ncp = (n1 >> 6) + 1
    total, sentinel, cp = [0, 0, 0, 0], -1, bytearray()
    for b in range(ncp):
        words = [0, 0, 0, 0]
        before = list(total)
        for j in range(64):
            r = 64 * b + j
            if r >= n1:
                break
            if sa[r] == 0:
                sentinel = r
                continue
            c = text[sa[r] - 1]
            words[c] |= 1 << (63 - j)
            total[c] += 1
        cp += struct.pack("<4q4Q", *before, *words)
    count = [1]
    for c in range(4):
        count.append(count[-1] + total[c])
    n_sa = (n1 >> 3) + 1 if sa_compx else n1
    ms, ls = bytearray(), bytearray()
    for i in range(n_sa):
        r = i << sa_compx
        v = sa[r] if r < n1 else 0
        ms += struct.pack("<B", v >> 32)
        ls += struct.pack("<I", v & 0xffffffff)
    return dict(ref_seq_len=n1, count=count, sentinel_index=sentinel, cp_occ=bytes(cp), ms=bytes(ms), ls=bytes(ls), sa=sa)


CODES = {"A": 0, "C": 1, "G": 2, "T": 3, "a": 0, "c": 1, "g": 2, "t": 3}


def parse_fasta(data):
    """FASTA bytes -> (codes, contigs [(name, comment, off, len, n_ambs)], holes [(off, len, char)]); raises ValueError."""
    rng = Rand48(11)
    codes, contigs, holes = [], [], []
    cur = None
    for raw in data.decode("latin-1").split("\n"):
        line = raw[:-1] if raw.endswith("\r") else raw
        if not line:
            continue
        if line[0] == ">":
            if cur is not None:
                if len(codes) == cur[2]:
                    raise ValueError("no bases")
                contigs.append((cur[0], cur[1], cur[2], len(codes) - cur[2], cur[3]))
            head = line[1:]
            k = 0
            while k < len(head) and not head[k].isspace():
                k += 1
            cur, last = [head[:k], head[k + 1:], len(codes), 0], ""
            continue
        if cur is None:
            raise ValueError("before any header")
        for ch in line:
            if not (33 <= ord(ch) <= 126):
                continue
            c = CODES.get(ch)
            if c is None:
                if ch == last:
                    holes[-1][1] += 1
                else:
                    holes.append([len(codes), 1, ch])
                    cur[3] += 1
                c = rng.next() & 3
            last = ch
            codes.append(c)
    if cur is None:
        raise ValueError("empty")
    if len(codes) == cur[2]:
        raise ValueError("no bases")
    contigs.append((cur[0], cur[1], cur[2], len(codes) - cur[2], cur[3]))
    return codes, contigs, [tuple(h) for h in holes]


def reference_files(data):
    """FASTA bytes -> {".ann": bytes, ".amb": bytes, ".pac": bytes, ".0123": bytes}, and the codes."""
    codes, contigs, holes = parse_fasta(data)
    L = len(codes)
    ann = "%d %d 11\n" % (L, len(contigs))
    for name, comment, off, ln, n_ambs in contigs:
        ann += "0 %s%s\n%d %d %d\n" % (name, " " + comment if comment else "", off, ln, n_ambs)
    amb = "%d %d %d\n" % (L, len(contigs), len(holes)) + "".join("%d %d %s\n" % h for h in holes)
    pac = bytearray((L + 3) // 4)
    for l, c in enumerate(codes):
        pac[l >> 2] |= c << ((~l & 3) << 1)
    if L % 4 == 0:
        pac.append(0)
    pac.append(L % 4)
    return {".ann": ann.encode("latin-1"), ".amb": amb.encode("latin-1"), ".pac": bytes(pac), ".0123": bytes(text_of(codes))}, codes
