"""Host side of the dbg assembly stage (include/gbx.h, dbg_asm section): per window the cycle check, the rebuild at a larger
k while the graph is cyclic, and the variant paths of the final graph.  ``assemble_host`` / ``DeviceAsm`` call libgbx.so,
where every graph is built, checked and searched on the GPU; ``Result.window`` gives one window in the shape of the tests'
restatement.  The reads and windows are dbg.py's (DbgReads, DbgWins)."""
import ctypes as C

import numpy as np

from . import _native as N
from . import dbg as D

OK, GAVE_UP, STEPS = 0, 1, 2
MAX_PENDING = 59
WIN_DTYPE = np.dtype([("k", "<i4"), ("n_builds", "<i4"), ("cyclic", "<i4"), ("pad_", "<i4"), ("first_start", "<i8"), ("n_starts", "<i8"),
                      ("n_paths", "<i8"), ("n_path_nodes", "<i8"), ("n_gave_up", "<i8"), ("n_steps", "<i8")])
START_DTYPE = np.dtype([("first_path", "<i8"), ("n_paths", "<i8"), ("first_node", "<i8"), ("n_nodes", "<i8"), ("win", "<i4"), ("node", "<i4"),
                        ("edge", "<i4"), ("status", "<i4")])
PATH_DTYPE = np.dtype([("weight", "<i8"), ("first_node", "<i8"), ("n_nodes", "<i4"), ("pos_first", "<i4"), ("pos_last", "<i4"), ("pad_", "<i4")])


class AsmParams(C.Structure):              # gbx_dbg_asm_params
    _fields_ = [("min_weight", C.c_int32), ("k_step", C.c_int32), ("k_last", C.c_int32), ("max_pending", C.c_int32), ("max_finished", C.c_int32),
                ("pad_", C.c_int32), ("max_steps", C.c_int64)]


class AsmOutC(C.Structure):                # gbx_dbg_asm_out
    _fields_ = [(f, C.c_void_p) for f in ("stats", "wins", "starts", "paths", "path_nodes", "path_seq")] + \
               [(f, C.c_int64) for f in ("cap_starts", "cap_paths", "cap_path_nodes")] + [("totals", C.c_void_p)]


def make_asm_params(min_weight=40, k_step=5, k_last=50, max_pending=20, max_finished=20, max_steps=1 << 20):
    return AsmParams(int(min_weight), int(k_step), int(k_last), int(max_pending), int(max_finished), 0, int(max_steps))


class Result:
    """One call's output: stats STATS_DTYPE[n_win], wins WIN_DTYPE[n_win], starts, paths, path_nodes int32, path_seq uint8."""

    def __init__(self, stats, wins, starts, paths, path_nodes, path_seq):
        self.stats, self.wins, self.starts, self.paths, self.path_nodes, self.path_seq = stats, wins, starts, paths, path_nodes, path_seq

    def window(self, w):
        """window w as the restatement's dict (tests/dbg_asm_ref.py window(), without its graph and step counts)"""
        ww = self.wins[w]
        out = {f: int(ww[f]) for f in ("k", "n_builds", "cyclic", "n_paths", "n_path_nodes", "n_gave_up", "n_steps")}
        out["stats"] = {f: int(self.stats[w][f]) for f in D.STATS_FIELDS}
        out["starts"] = []
        for s in range(int(ww["first_start"]), int(ww["first_start"]) + int(ww["n_starts"])):
            sr = self.starts[s]
            paths = []
            for x in range(int(sr["first_path"]), int(sr["first_path"]) + int(sr["n_paths"])):
                pa = self.paths[x]
                a, b = int(pa["first_node"]), int(pa["first_node"]) + int(pa["n_nodes"])
                paths.append(dict(nodes=[int(v) for v in self.path_nodes[a:b]], weight=int(pa["weight"]), pos_first=int(pa["pos_first"]),
                                  pos_last=int(pa["pos_last"]), seq=self.path_seq[a:b].tobytes()))
            out["starts"].append(dict(win=int(sr["win"]), node=int(sr["node"]), edge=int(sr["edge"]), status=int(sr["status"]),
                                      first_node=int(sr["first_node"]), n_nodes=int(sr["n_nodes"]), paths=paths))
        return out


def window_line(res, w):
    """One line of `dbg --assemble`: final k, builds, cyclic, starts, paths, give-ups"""
    ww = res.wins[w]
    return "%d\t%d\t%d\t%d\t%d\t%d" % tuple(int(ww[f]) for f in ("k", "n_builds", "cyclic", "n_starts", "n_paths", "n_gave_up"))


def assemble_host(reads, wins, params=None, asm_params=None, caps=(1024, 1024, 1 << 16)):
    """gbx_dbg_assemble_host -> Result; where a capacity is short the call is repeated with what it asked for."""
    p, ap = params or D.make_params(), asm_params or make_asm_params()
    r, w = reads.c_struct(), wins.c_struct()
    nw = max(wins.n_win, 1)
    caps = [max(int(c), 1) for c in caps]
    for _ in range(4):
        st, wn = np.zeros(nw, dtype=D.STATS_DTYPE), np.zeros(nw, dtype=WIN_DTYPE)
        starts, paths = np.zeros(caps[0], dtype=START_DTYPE), np.zeros(caps[1], dtype=PATH_DTYPE)
        pn, ps = np.zeros(caps[2], dtype=np.int32), np.zeros(caps[2], dtype=np.uint8)
        tot = np.zeros(3, dtype=np.int64)
        o = AsmOutC(N.ptr(st), N.ptr(wn), N.ptr(starts), N.ptr(paths), N.ptr(pn), N.ptr(ps), caps[0], caps[1], caps[2], N.ptr(tot))
        rc = N.lib().gbx_dbg_assemble_host(C.byref(p), C.byref(ap), C.byref(r), C.byref(w), C.byref(o))
        if rc == N.GBX_ERR_UNSUPPORTED and any(int(t) > c for t, c in zip(tot, caps)):
            caps = [max(c, int(t)) for t, c in zip(tot, caps)]
            continue
        N.check(rc)
        return Result(st[:wins.n_win], wn[:wins.n_win], starts[:tot[0]], paths[:tot[1]], pn[:tot[2]], ps[:tot[2]])
    raise RuntimeError("gbx_dbg_assemble_host: the capacities did not settle")


class DeviceAsm:
    """Reads and windows on a device (dbg.DeviceDbg's arrays); assemble() = one gbx_dbg_assemble_device call on `stream`."""

    def __init__(self, reads, wins, device, params=None, asm_params=None, caps=(1024, 1024, 1 << 16), work_bytes=None):
        import torch
        self.p, self.ap = params or D.make_params(), asm_params or make_asm_params()
        self.base = D.DeviceDbg(reads, wins, device, self.p, work_bytes=1)
        self.dev, self.n_win = self.base.dev, wins.n_win
        occ = wins.occ_slots(reads, self.p.k)
        self.work_bytes = N.lib().gbx_dbg_assemble_workspace_bytes(C.byref(self.p), wins.n_win, reads.n_reads, int(occ.max()) if occ.size else 0)
        if work_bytes is not None:           # a smaller workspace: more, smaller ranges of windows (at least the largest window)
            self.work_bytes = int(work_bytes)
        self.work = torch.empty(max(self.work_bytes, 1), dtype=torch.uint8, device=self.dev)
        self.caps = [max(int(c), 1) for c in caps]
        nw = max(wins.n_win, 1)
        z = lambda n: torch.zeros(n, dtype=torch.uint8, device=self.dev)  # noqa: E731
        self.bufs = [z(nw * D.STATS_DTYPE.itemsize), z(nw * WIN_DTYPE.itemsize), z(self.caps[0] * START_DTYPE.itemsize),
                     z(self.caps[1] * PATH_DTYPE.itemsize), z(self.caps[2] * 4), z(self.caps[2]), z(24)]
        self.out = AsmOutC(*(b.data_ptr() for b in self.bufs[:6]), self.caps[0], self.caps[1], self.caps[2], self.bufs[6].data_ptr())

    def assemble(self, stream=None):
        """-> the entry's return value (GBX_ERR_UNSUPPORTED: a capacity was short, see totals()); other errors raise"""
        rc = N.lib().gbx_dbg_assemble_device(C.byref(self.p), C.byref(self.ap), C.byref(self.base.reads), C.byref(self.base.wins),
                                             C.byref(self.out), self.work.data_ptr(), self.work_bytes, stream)
        if rc != N.GBX_ERR_UNSUPPORTED:
            N.check(rc)
        return rc

    def totals(self):
        return [int(x) for x in self.bufs[6].cpu().numpy().view(np.int64)]

    def results(self):
        h = [b.cpu().numpy() for b in self.bufs[:6]]
        tot = [min(t, c) for t, c in zip(self.totals(), self.caps)]
        return Result(h[0].view(D.STATS_DTYPE)[:self.n_win].copy(), h[1].view(WIN_DTYPE)[:self.n_win].copy(), h[2].view(START_DTYPE)[:tot[0]].copy(),
                      h[3].view(PATH_DTYPE)[:tot[1]].copy(), h[4].view(np.int32)[:tot[2]].copy(), h[5][:tot[2]].copy())
