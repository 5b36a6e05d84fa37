"""Reads in, SAM out: the whole bwa-mem path behind one call, gbx_mem_index / gbx_mem_aligner (include/gbx.h).

``MemIndex`` uploads an index once (the FM index with its suffix-array samples, the 2 L-byte text, the contigs and their names);
``MemAligner(index).run(readset, names, qual, id0)`` queues smem -> sal -> chain -> extend -> regs -> [pestat -> rescue ->] pair ->
cigar -> sam on the aligner's own stream, reads every count once, runs the chain again from the first stage whose capacity was
too small, and returns the SAM lines, the records and the statistics.  ``plan`` is the host-only capacity planner.
``save_reference`` writes the .ann / .pac / .0123 files the ``mem`` driver reads beside ``fmi.save_bwa_mem2_index``'s file.
"""
import ctypes as C

import numpy as np

from . import _native as N
from . import fmi as FM
from . import mem_chain as MC
from . import mem_cigar as MG
from . import mem_pair as MP
from . import mem_regs as MR
from . import mem_rescue as MS
from . import mem_sam as SM
from .bsw_seeds import SeedParams
from .mem_pair import PESTAT_DTYPE
from .mem_sam import SAM_DTYPE

MAX_RERUNS = 64
STAGES = ("smem", "sal", "chain", "extend", "regs", "pestat", "rescue", "pair", "cigar", "sam")
CAP_FIELDS = ("slot", "out_cap", "pos_cap", "chain_cap", "seed_cap", "reg_cap", "sel_cap", "xreg_cap", "xseed_cap", "xsel_cap", "psel_cap",
              "cigar_cap", "z_bytes", "rec_cap", "md_cap", "text_cap")
COUNT_FIELDS = ("slot_worst", "n_smem", "n_pos", "n_chains", "n_seeds", "n_regs", "n_sel", "n_xregs", "n_xseeds", "n_xsel", "n_psel",
                "n_cigar", "n_z_miss", "n_recs", "n_md", "n_text", "n_alns", "pad_")


class Pestat(C.Structure):               # gbx_mem_pestat
    _fields_ = [("low", C.c_int32), ("high", C.c_int32), ("failed", C.c_int32), ("pad_", C.c_int32), ("avg", C.c_double), ("std", C.c_double)]


class AlignParams(C.Structure):          # gbx_mem_align_params
    _fields_ = [("fmi", FM.FmiParams), ("chain", MC.ChainParams), ("bsw", SeedParams), ("regs", MR.RegsParams), ("pair", MP.PairParams),
                ("rescue", MS.RescueParams), ("cigar", MG.CigarParams), ("sam", SM.SamParams), ("max_occ", C.c_int32), ("mode", C.c_int32),
                ("have_pes", C.c_int32), ("no_rescue", C.c_int32), ("pes", Pestat * 4)]


class AlignCaps(C.Structure):            # gbx_mem_align_caps
    _fields_ = [(n, C.c_int64) for n in CAP_FIELDS]


class AlignCounts(C.Structure):          # gbx_mem_align_counts
    _fields_ = [(n, C.c_int64) for n in COUNT_FIELDS]


class AlignStats(C.Structure):           # gbx_mem_align_stats
    _fields_ = [("counts", AlignCounts), ("caps", AlignCaps), ("runs", C.c_int64), ("bytes_up", C.c_int64), ("bytes_down", C.c_int64),
                ("reruns", C.c_int32), ("slot_reruns", C.c_int32), ("rerun_stage", C.c_int32 * MAX_RERUNS)]


class AlignOut(C.Structure):             # gbx_mem_align_out
    _fields_ = [("sam", C.c_void_p), ("n_text", C.c_int64), ("recs", C.c_void_p), ("n_recs", C.c_int64), ("rec_off", C.c_void_p),
                ("pes", Pestat * 4), ("stats", AlignStats)]


@N.declare_once
def lib(L):
    """libgbx.so with the aligner's entries declared (raises if the library or the entries are missing)."""
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    PP, PC, PN = C.POINTER(AlignParams), C.POINTER(AlignCaps), C.POINTER(AlignCounts)
    L.gbx_mem_align_sizes.argtypes = [C.POINTER(i64)]
    L.gbx_mem_align_sizes.restype = None
    L.gbx_mem_align_default_params.argtypes = [PP]
    L.gbx_mem_align_default_params.restype = None
    L.gbx_mem_align_set_scoring.argtypes = [PP] + [i32] * 13
    L.gbx_mem_align_set_scoring.restype = None
    L.gbx_mem_align_check_params.argtypes = [PP]
    L.gbx_mem_align_plan.argtypes = [PP, i64, i64, i32, i64, PN, i64, PC]
    L.gbx_mem_index_create.argtypes = [vp, vp, vp, i64, i32, vp, vp, vp, C.POINTER(vp)]
    L.gbx_mem_index_build.argtypes = [vp, i64, i32, vp, vp, vp, C.POINTER(vp)]
    L.gbx_mem_index_destroy.argtypes = [vp]
    L.gbx_mem_index_destroy.restype = None
    L.gbx_mem_sam_header.argtypes = [vp, vp, i64, C.POINTER(i64)]
    L.gbx_mem_aligner_create.argtypes = [vp, PP, PC, C.POINTER(vp)]
    L.gbx_mem_aligner_destroy.argtypes = [vp]
    L.gbx_mem_aligner_destroy.restype = None
    L.gbx_mem_aligner_run.argtypes = [vp, i64, i64, vp, i64, vp, vp, vp, vp, vp, C.POINTER(AlignOut)]
    L.gbx_mem_aligner_stats.argtypes = [vp, C.POINTER(AlignStats)]
    L.gbx_mem_pair_device_pes.argtypes = MP.lib().gbx_mem_pair_device.argtypes


def sizes():
    """gbx_mem_align_sizes: sizeof of (params, caps, counts, stats, out)."""
    out = (C.c_int64 * 5)()
    lib().gbx_mem_align_sizes(out)
    return tuple(int(x) for x in out)


def default_params(mode=1):
    p = AlignParams()
    lib().gbx_mem_align_default_params(C.byref(p))
    p.mode = int(mode)
    return p


def set_scoring(p, a=1, b=4, o_del=6, e_del=1, o_ins=6, e_ins=1, pen_clip5=5, pen_clip3=5, pen_unpaired=17, w=100, zdrop=100,
                min_seed_len=19, T=30):
    """gbx_mem_align_set_scoring: every copy of these values in the stage structs of `p` (defaults: bwa mem's)."""
    lib().gbx_mem_align_set_scoring(C.byref(p), a, b, o_del, e_del, o_ins, e_ins, pen_clip5, pen_clip3, pen_unpaired, w, zdrop, min_seed_len, T)
    return p


def set_pes(p, pes):
    """A caller's estimate (bwa -I): four (low, high, failed, avg, std) or a PESTAT_DTYPE array; None takes it out."""
    rec = MP.pestat_records(pes)
    p.have_pes = 0 if rec is None else 1
    for d in range(4):
        if rec is None:
            p.pes[d] = Pestat(0, 0, 1, 0, 0., 0.)
        else:
            p.pes[d] = Pestat(int(rec[d]["low"]), int(rec[d]["high"]), int(rec[d]["failed"]), 0, float(rec[d]["avg"]), float(rec[d]["std"]))
    return p


def check_params(p):
    """gbx_mem_align_check_params: raises GbxError when two copies of a value disagree."""
    N.check(lib().gbx_mem_align_check_params(C.byref(p)))


def caps_dict(c):
    return {n: int(getattr(c, n)) for n in CAP_FIELDS}


def counts_dict(c):
    return {n: int(getattr(c, n)) for n in COUNT_FIELDS if n != "pad_"}


def make_caps(**kw):
    c = AlignCaps()
    for k, v in kw.items():
        if k not in CAP_FIELDS:
            raise TypeError("gbx_mem_align_caps has no field %r" % k)
        setattr(c, k, int(v))
    return c


def plan(params, n_reads, bases, max_read_len, name_bytes, last=None, last_bases=0):
    """gbx_mem_align_plan -> AlignCaps.  last: an AlignCounts (or a dict of its fields) of an earlier batch of last_bases bases."""
    if isinstance(last, dict):
        d, last = last, AlignCounts()
        for k, v in d.items():
            setattr(last, k, int(v))
    c = AlignCaps()
    N.check(lib().gbx_mem_align_plan(C.byref(params), int(n_reads), int(bases), int(max_read_len), int(name_bytes),
                                     C.byref(last) if last is not None else None, int(last_bases), C.byref(c)))
    return c


class MemIndex:
    """gbx_mem_index: everything of a reference on the device, made once and read-only afterwards (several aligners and threads
    may share it).  genome: base codes 0..3 of one strand, or an (FmiIndex, FmiSa) pair with `text` given; contig_off:
    int64[n_contigs + 1] from 0 to the genome's length; contig_names: one string per contig."""

    def __init__(self, genome, contig_off, contig_names, text=None):
        if isinstance(genome, tuple):
            idx, smp = genome
            assert text is not None, "an (FmiIndex, FmiSa) pair needs the text"
        else:
            idx, smp = FM.build_index(genome, sa_compx=3)
            text = MC.text_of(genome)
        idx, smp = idx.host(), smp.host()
        text = np.ascontiguousarray(text, dtype=np.uint8)
        co = np.ascontiguousarray(contig_off, dtype=np.int64)
        cn, cno = SM.arena(contig_names)
        self.l_pac, self.contig_off, self.contig_names = len(text) // 2, co, [x.decode() if isinstance(x, bytes) else str(x) for x in contig_names]
        st = idx.struct(idx.cp_occ.ctypes.data)
        sst = smp.struct(*smp.ptrs())
        h = C.c_void_p()
        N.check(lib().gbx_mem_index_create(C.addressof(st), C.addressof(sst), N.ptr(text), self.l_pac, len(co) - 1, N.ptr(co),
                                           N.ptr(cn) if len(cn) else None, N.ptr(cno), C.byref(h)))
        self.handle = h

    @classmethod
    def build(cls, genome, contig_off, contig_names):
        """gbx_mem_index_build: the same index from the genome alone, built on the device (sa_compx 3); nothing of it comes back to
        the host."""
        g = np.ascontiguousarray(genome, dtype=np.uint8)
        co = np.ascontiguousarray(contig_off, dtype=np.int64)
        cn, cno = SM.arena(contig_names)
        self = cls.__new__(cls)
        self.handle = None
        self.l_pac, self.contig_off, self.contig_names = len(g), co, [x.decode() if isinstance(x, bytes) else str(x) for x in contig_names]
        h = C.c_void_p()
        N.check(lib().gbx_mem_index_build(N.ptr(g) if len(g) else None, len(g), len(co) - 1, N.ptr(co), N.ptr(cn) if len(cn) else None, N.ptr(cno),
                                          C.byref(h)))
        self.handle = h
        return self

    def header(self):
        """gbx_mem_sam_header: the @SQ lines as bytes."""
        need = C.c_int64(0)
        lib().gbx_mem_sam_header(self.handle, None, 0, C.byref(need))
        buf = np.zeros(max(need.value, 1), dtype=np.uint8)
        N.check(lib().gbx_mem_sam_header(self.handle, N.ptr(buf), len(buf), C.byref(need)))
        return buf[:need.value].tobytes()

    def close(self):
        if self.handle:
            lib().gbx_mem_index_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _stats(s):
    n = min(int(s.reruns), MAX_RERUNS)
    return dict(counts=counts_dict(s.counts), caps=caps_dict(s.caps), runs=int(s.runs), bytes_up=int(s.bytes_up), bytes_down=int(s.bytes_down),
                reruns=int(s.reruns), slot_reruns=int(s.slot_reruns), rerun_stage=[int(s.rerun_stage[k]) for k in range(n)])


class MemAligner:
    """gbx_mem_aligner on a MemIndex: one stream, all stage buffers, pinned buffers for its input and output.  One thread at a
    time; several aligners may run at once on one index."""

    def __init__(self, index, params=None, first_caps=None):
        self.index = index                # kept alive: the aligner reads it
        self.params = params or default_params()
        h = C.c_void_p()
        N.check(lib().gbx_mem_aligner_create(index.handle, C.byref(self.params), C.byref(first_caps) if first_caps is not None else None,
                                             C.byref(h)))
        self.handle = h

    def run(self, reads, names, qual=None, id0=0):
        """reads: an ``fmi.FmiReadSet``; names: one string per read; qual: uint8 at the reads' offsets or None; id0: the first
        pair's id (mode 1) or read's (mode 0).  -> dict(sam bytes, recs SAM_DTYPE[n_recs], rec_off int64[n_reads + 1], pes
        PESTAT_DTYPE[4], stats dict).  Raises GbxError on a refusal."""
        nm, no = SM.arena(names)
        assert len(no) == reads.n_reads + 1
        q = None if qual is None else np.ascontiguousarray(qual, dtype=np.uint8)
        assert q is None or len(q) == len(reads.enc)
        return self.run_arrays(reads.n_reads, reads.enc, reads.read_off, reads.read_len, q, nm, no, id0)

    def run_arrays(self, n_reads, enc, read_off, read_len, qual, name_arena, name_off, id0=0):
        """gbx_mem_aligner_run on the arrays as they are (numpy, C-contiguous; qual may be None)."""
        out = AlignOut()
        keep = np.zeros(2, np.int64)
        opt = lambda a: N.ptr(a) if a is not None and len(a) else None
        N.check(lib().gbx_mem_aligner_run(self.handle, int(n_reads), int(id0), opt(enc) or N.ptr(keep), len(enc), opt(read_off) or N.ptr(keep),
                                          opt(read_len) or N.ptr(keep), opt(qual), opt(name_arena), N.ptr(name_off), C.byref(out)))
        sam = C.string_at(out.sam, out.n_text) if out.n_text else b""
        recs = np.frombuffer(C.string_at(out.recs, out.n_recs * SAM_DTYPE.itemsize), dtype=SAM_DTYPE).copy() if out.n_recs else np.zeros(0, SAM_DTYPE)
        rec_off = np.frombuffer(C.string_at(out.rec_off, (int(n_reads) + 1) * 8), dtype=np.int64).copy()
        pes = np.zeros(4, dtype=PESTAT_DTYPE)
        for d in range(4):
            pes[d] = (out.pes[d].low, out.pes[d].high, out.pes[d].failed, out.pes[d].pad_, out.pes[d].avg, out.pes[d].std)
        return dict(sam=sam, recs=recs, rec_off=rec_off, pes=pes, stats=_stats(out.stats))

    def stats(self):
        s = AlignStats()
        N.check(lib().gbx_mem_aligner_stats(self.handle, C.byref(s)))
        return _stats(s)

    def header(self):
        return self.index.header()

    def close(self):
        if self.handle:
            lib().gbx_mem_aligner_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def save_reference(prefix, genome, contig_off, contig_names):
    """Writes <prefix>.ann, <prefix>.pac and <prefix>.0123 in bwa's layouts (UNPINNED: nothing of bwa-mem2 can be built or run
    here), beside the <prefix>.bwt.2bit.64 that ``fmi.save_bwa_mem2_index`` writes.
      .ann   "l_pac n_seqs seed", then per contig "gi name [comment]" and "offset len n_ambs"
      .pac   2 bits per base, the first base in the top bits of a byte: base l = pac[l >> 2] >> ((~l & 3) << 1) & 3; then, as bwa
             writes it, a zero byte when l_pac is a multiple of 4, and a byte l_pac % 4
      .0123  2 l_pac bytes of codes 0..3: the genome, then its reverse complement"""
    g = np.ascontiguousarray(genome, dtype=np.uint8)
    co = np.asarray(contig_off, dtype=np.int64)
    L = len(g)
    assert len(co) == len(contig_names) + 1 and co[0] == 0 and co[-1] == L and g.max(initial=0) < 4
    with open("%s.ann" % prefix, "w") as f:
        f.write("%d %d %d\n" % (L, len(contig_names), 11))
        for k, n in enumerate(contig_names):
            f.write("0 %s\n%d %d 0\n" % (n.decode() if isinstance(n, bytes) else n, int(co[k]), int(co[k + 1] - co[k])))
    pad = np.zeros((L + 3) // 4 * 4, dtype=np.uint8)
    pad[:L] = g
    q = pad.reshape(-1, 4)
    pac = (q[:, 0] << 6 | q[:, 1] << 4 | q[:, 2] << 2 | q[:, 3]).astype(np.uint8)
    with open("%s.pac" % prefix, "wb") as f:
        f.write(pac.tobytes())
        if L % 4 == 0:
            f.write(b"\0")
        f.write(bytes([L % 4]))
    with open("%s.0123" % prefix, "wb") as f:
        f.write(MC.text_of(g).tobytes())
