"""A plain-Python restatement of the dbg contract (include/gbx.h, dbg section): the windows and their reads, and
one de Bruijn graph per window in a dict kept in insertion order, with lists of at most 4 edges.  Independent of the
device code and of the reference's source."""
import struct

FNV_BASIS, FNV_PRIME, MASK64 = 0xcbf29ce484222325, 0x100000001b3, (1 << 64) - 1
REF, READ = 1, 2
STATS_FIELDS = ("n_nodes", "n_edges", "n_dropped", "n_occ", "weight_sum", "n_ref", "n_read", "n_both", "digest")


def windows(pos, end, beg, stop, region_size=1500):
    """-> [(assem_start, assem_end, ref_start, ref_end, lo, hi)]; raises ValueError((w, start, end, lo, hi)) where the
    reference stops (lo > hi).  pos / end: the reads' uint32 values in file order."""
    pos, end = [int(x) for x in pos], [int(x) for x in end]
    n = len(pos)
    shift = max(100, min(1000, region_size // 2))
    longest = 0
    for p, e in zip(pos, end):
        d = (e - p) & 0xffffffff
        longest = max(longest, d - (1 << 32) if d >= 1 << 31 else d)

    def bisect(x):
        a, b = 0, n
        while a < b:
            m = (a + b) // 2
            if pos[m] < x:
                a = m + 1
            else:
                b = m
        return a
    out = []
    k = beg
    while k < stop:
        a0, a1 = k, min(k + region_size, stop)
        f0, f1 = max(0, k - region_size), a1 + region_size
        lo = hi = 0
        if n:
            first = max(1, a0 - longest)
            lo, hi = bisect(first & 0xffffffff), bisect(a1 & 0xffffffff)
            while lo < n and end[lo] <= a0:
                lo += 1
        if lo > hi:
            raise ValueError((len(out), a0, a1, lo, hi))
        out.append((a0, a1, f0, f1, lo, min(hi, n)))
        k += shift
    return out


def graph(ref, ref_pos, reads, k=15, min_qual=20):
    """ref: bytes; reads: [(seq bytes, qual bytes, flag)] of the window in order.
    -> (nodes, stats): nodes a list in first-touch order of dicts kmer, colours, position, weight, src, edges [[end index,
    weight]] (src: ('ref', offset) or ('read', read index, offset) of the first touch)."""
    nodes = {}                 # kmer -> node dict (insertion order = first touch)
    occ = wsum = dropped = 0

    def touch(km, colour, position, weight, src):
        nd = nodes.get(km)
        if nd is None:
            nd = dict(kmer=km, colours=colour, position=position, weight=weight, src=src, succ=[], index=len(nodes))
            nodes[km] = nd
        else:
            nd["colours"] |= colour
            nd["weight"] += weight
        return nd

    def add(seq, i, colour, position, weight, src_of):
        nonlocal occ, wsum, dropped
        a = touch(seq[i:i + k], colour, position, weight, src_of(i))
        b = touch(seq[i + 1:i + 1 + k], colour, position + 1 if position >= 0 else -1, weight, src_of(i + 1))
        occ += 1
        wsum += weight
        for e in a["succ"]:
            if e[0] is b:
                e[1] += weight
                return
        if len(a["succ"]) < 4:
            a["succ"].append([b, weight])
        else:
            a.setdefault("extra", set()).add(b["kmer"])

    for i in range(len(ref) - k - 1):
        add(ref, i, REF, ref_pos + i, 1, lambda j: ("ref", j))
    for r, (seq, qual, flag) in enumerate(reads):
        if flag & 0x200:
            continue
        for i in range(len(seq) - k - 1):
            win = seq[i:i + k + 1]
            if b"N" in win:
                continue
            q = min(qual[i:i + k + 1])
            if q < min_qual:
                continue
            add(seq, i, READ, -1, q, lambda j, r=r: ("read", r, j))
    out = []
    for nd in nodes.values():
        out.append(dict(kmer=nd["kmer"], colours=nd["colours"], position=nd["position"], weight=nd["weight"], src=nd["src"],
                        edges=[[e[0]["index"], e[1]] for e in nd["succ"]]))
        dropped += len(nd.get("extra", ()))
    st = dict(n_nodes=len(out), n_edges=sum(len(n["edges"]) for n in out), n_dropped=dropped, n_occ=occ, weight_sum=wsum,
              n_ref=sum(n["colours"] == REF for n in out), n_read=sum(n["colours"] == READ for n in out),
              n_both=sum(n["colours"] == REF | READ for n in out), digest=digest(out))
    return out, st


def record(nd):
    """A node's digest record (gbx.h): k bytes, colours u8, position i32, weight i64, n_edges u8, (end i32, weight i64)."""
    b = nd["kmer"] + struct.pack("<BiqB", nd["colours"], nd["position"], nd["weight"], len(nd["edges"]))
    for e, w in nd["edges"]:
        b += struct.pack("<iq", e, w)
    return b


def digest(nodes):
    h = FNV_BASIS
    for nd in nodes:
        for byte in record(nd):
            h = ((h ^ byte) * FNV_PRIME) & MASK64
    return h


def dump_window(nodes):
    """The text form of one window's graph the recorded reference dump uses: one line per node in first-touch order,
    'kmer colours position weight' then ' end:weight' per edge."""
    lines = []
    for nd in nodes:
        s = "%s %d %d %d" % (nd["kmer"].decode("latin-1"), nd["colours"], nd["position"], nd["weight"])
        s += "".join(" %d:%d" % (e, w) for e, w in nd["edges"])
        lines.append(s)
    return lines
