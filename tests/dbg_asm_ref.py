"""A plain-Python restatement of the dbg_asm contract (include/gbx.h, dbg_asm section) on the node lists of
tests/dbg_ref.py: the cycle check, the retry over k, the starts and the variant path search.  Iterative throughout (a
recursive walk dies on a line of a few thousand nodes).  Independent of the device code."""
import dbg_ref as R

REF, READ, BOTH = R.REF, R.READ, R.REF | R.READ
OK, GAVE_UP, STEPS = 0, 1, 2
DEFAULTS = dict(min_weight=40, k_step=5, k_last=50, max_pending=20, max_finished=20, max_steps=1 << 20)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def counted(nodes, end, weight, min_weight):
    """an edge the cycle check sees: not one of weight below min_weight into a READ-only node"""
    return not (nodes[end]["colours"] == READ and weight < min_weight)


def cyclic(nodes, min_weight):
    """detectCyclesInGraph_Recursive's answer, by a colouring walk with an explicit stack: a grey node reached again"""
    WHITE, GREY, BLACK = 0, 1, 2
    colour = [WHITE] * len(nodes)
    for root in range(len(nodes)):
        if colour[root] != WHITE:
            continue
        colour[root] = GREY
        stack = [(root, 0)]
        while stack:
            v, x = stack.pop()
            edges = nodes[v]["edges"]
            while x < len(edges) and not counted(nodes, edges[x][0], edges[x][1], min_weight):
                x += 1
            if x == len(edges):
                colour[v] = BLACK
                continue
            stack.append((v, x + 1))
            e = edges[x][0]
            if colour[e] == GREY:
                return True
            if colour[e] == WHITE:
                colour[e] = GREY
                stack.append((e, 0))
    return False


def starts(nodes, min_weight):
    """[(node, edge number)] in first-touch order, then edge order (UPSTREAM: Platypus's findBubbles)"""
    return [(i, j) for i, nd in enumerate(nodes) if nd["colours"] == BOTH for j, (e, w) in enumerate(nd["edges"])
            if nodes[e]["colours"] == READ and w >= min_weight]


def search(nodes, node, edge, p):
    """getVariantPathsThroughGraphFromNode from one start -> (status, [(node list, weight)] in finishing order, steps, the most
    paths left on the stack behind a pop)"""
    e, w = nodes[node]["edges"][edge]
    stack, fin, steps, peak = [([node, e], w)], [], 0, 0
    while stack:
        path, wt = stack.pop()
        steps += 1
        if steps > p["max_steps"]:
            return STEPS, [], steps, peak
        peak = max(peak, len(stack))
        if len(stack) > p["max_pending"] or len(fin) > p["max_finished"]:
            return GAVE_UP, [], steps, peak
        last = nodes[path[-1]]
        if path[-1] in path[:-1]:
            continue
        if last["colours"] == BOTH:
            fin.append((path, wt))
        elif last["colours"] == REF:
            continue
        else:
            for e, w in last["edges"]:
                if w >= p["min_weight"] or nodes[e]["colours"] & REF:
                    stack.append((path + [e], wt + w))
    return OK, fin, steps, peak


def window(ref, ref_pos, reads, k=15, min_qual=20, p=None):
    """One window from its first graph to its paths -> dict: k, n_builds, cyclic, stats, nodes (the final graph), starts
    [dict node, edge, status, steps, peak, paths [dict nodes, weight, pos_first, pos_last, seq]] and the counts."""
    p = p or params()
    n_builds = 0
    while True:
        nodes, st = R.graph(ref, ref_pos, reads, k, min_qual)
        n_builds += 1
        cyc = cyclic(nodes, p["min_weight"])
        if not cyc or k > p["k_last"]:
            break
        k += p["k_step"]
    out = dict(k=k, n_builds=n_builds, cyclic=int(cyc), stats=st, nodes=nodes, starts=[], n_paths=0, n_path_nodes=0, n_gave_up=0, n_steps=0)
    for i, j in starts(nodes, p["min_weight"]):
        status, fin, steps, peak = search(nodes, i, j, p)
        paths = [dict(nodes=path, weight=wt, pos_first=nodes[path[0]]["position"], pos_last=nodes[path[-1]]["position"],
                      seq=bytes(nodes[v]["kmer"][0] for v in path)) for path, wt in fin]
        out["starts"].append(dict(node=i, edge=j, status=status, steps=steps, peak=peak, paths=paths))
        out["n_paths"] += len(paths)
        out["n_path_nodes"] += sum(len(x["nodes"]) for x in paths)
        out["n_gave_up"] += status == GAVE_UP
        out["n_steps"] += status == STEPS
    return out


def line(w):
    """the driver's --assemble line of one window (tab separated): final k, builds, cyclic, starts, paths, give-ups"""
    return "%d\t%d\t%d\t%d\t%d\t%d" % (w["k"], w["n_builds"], w["cyclic"], len(w["starts"]), w["n_paths"], w["n_gave_up"])


def path_lines(w):
    """with --print, behind a window's line: one line per path: P, start position, end position, weight, sequence"""
    return ["P\t%d\t%d\t%d\t%s" % (x["pos_first"], x["pos_last"], x["weight"], x["seq"].decode("latin-1")) for s in w["starts"] for x in s["paths"]]
