"""The three dbg device entries - gbx_dbg_build_device, gbx_dbg_graph_device, gbx_dbg_assemble_device - read the offsets and
ranges back through one function and check them as the host entries check theirs (csrc/dbg_host.h), in front of the first
launch: with one device array spoiled at a time each returns GBX_ERR_ARG, and the next call on the same object, the array
mended, gives the restatement's result."""
import ctypes

import pytest

import dbg_asm_cases as AC
from genomicsbench_amd import _native as N
from genomicsbench_amd import dbg_asm as A
from test_dbg_asm_gpu import same
from test_dbg_edges_gpu import same_graph, same_stats

pytestmark = pytest.mark.gpu
SEQ_OFF, REF_OFF, READ_LO, READ_HI = 0, 4, 7, 8          # DeviceDbg.arrays


def test_spoiled_device_arrays_are_refused_before_the_first_launch():
    import torch
    case = {c.name: c for c in AC.all_cases()}["snp_k3"]
    rs, ws, p = case.packed()
    assert ws.n_win == 1 and case.k == 3 and rs.n_reads >= 1
    da = A.DeviceAsm(rs, ws, "cuda:0", p, case.asm_params())
    dd = da.base                                         # the same device arrays; a workspace of its own for the build
    dd.work_bytes = N.lib().gbx_dbg_workspace_bytes(ctypes.byref(p), ws.n_win, rs.n_reads, int(ws.occ_slots(rs, case.k).max()))
    dd.work = torch.empty(dd.work_bytes, dtype=torch.uint8, device=dd.dev)
    stream = torch.cuda.current_stream().cuda_stream
    want_st = case.want()[0]
    dd.build(stream)
    torch.cuda.synchronize()
    stats = dd.results()
    same_stats(stats, want_st, "snp_k3 before")
    spoils = [("read_lo = 1, read_hi = 0", [(READ_LO, 0, 1), (READ_HI, 0, 0)], "its reads are not"),
              ("read_hi = n_reads + 1", [(READ_HI, 0, rs.n_reads + 1)], "its reads are not"),
              ("ref_off decreasing", [(REF_OFF, 0, int(ws.ref.size)), (REF_OFF, 1, 0)], "ref_off decreases"),
              ("seq_off[n] > seq_bytes", [(SEQ_OFF, rs.n_reads, int(rs.seq.size) + 1)], "seq_off outside")]
    for what, changes, text in spoils:
        saved = [int(dd.arrays[a][i]) for a, i, _ in changes]
        for a, i, v in changes:
            dd.arrays[a][i] = v
        dd.stats.fill_(0xAB)
        marks = [b.fill_(0xCD) for b in da.bufs[:6]]
        torch.cuda.synchronize()
        for name, call in (("build", lambda: dd.build(stream)), ("graph", lambda: dd.graph(stats, 0, 1, stream)), ("assemble", lambda: da.assemble(stream))):
            with pytest.raises(N.GbxError) as e:
                call()
            assert e.value.code == N.GBX_ERR_ARG and text in str(e.value), (what, name, str(e.value))
        torch.cuda.synchronize()
        # nothing was launched: no output byte was written
        assert bool((dd.stats == 0xAB).all()) and all(bool((b == 0xCD).all()) for b in marks), what
        for (a, i, _), v in zip(changes, saved):
            dd.arrays[a][i] = v
        # the same objects, mended
        dd.build(stream)
        torch.cuda.synchronize()
        same_stats(dd.results(), want_st, "snp_k3 after " + what)
        same_graph(case, dd.graph(stats, 0, 1, stream), 0, 1, "snp_k3 graph after " + what)
        assert da.assemble(stream) == 0
        torch.cuda.synchronize()
        same(da.results(), case.want_asm(), "snp_k3 assemble after " + what)
