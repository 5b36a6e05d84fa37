"""The one composition of the bwa-mem stage classes: fmi (smem + sal) -> chain -> extend -> regs -> rescue -> pair -> cigar -> sam
on one stream.  ``Stages`` builds each stage behind the one before it (the records of ``mem_stage`` say what it hands on), queues
any range of them, hands out the steps for timing, checks every stage's capacities and sizes them from a run's counts.
``mem_rescue.pipeline``, ``mem_sam.pipeline``, the aligner's tests and scripts/time_mem_*.py all queue through it.
"""
from . import _native as N
from . import bsw_seeds as BS
from . import mem_chain as MC
from . import mem_cigar as MG
from . import mem_pair as MP
from . import mem_regs as MR
from . import mem_rescue as MS
from . import mem_sam as SM

ORDER = ("fmi", "chain", "extend", "regs", "rescue", "pair", "cigar", "sam")
# a stage's capacity arguments, and the counts it leaves on the device in their order there
CAPS = {"chain": ("chain_cap", "seed_cap"), "regs": ("reg_cap", "sel_cap"), "rescue": ("xreg_cap", "xseed_cap", "xsel_cap"),
        "pair": ("psel_cap",), "cigar": ("cigar_cap", "z_bytes"), "sam": ("rec_cap", "md_cap", "text_cap", "max_recs", "max_del")}
COUNTS = {"fmi": ("n_smem", "n_pos"), "chain": ("n_chains", "n_seeds"), "regs": ("n_regs", "n_sel"),
          "rescue": ("n_xregs", "n_xsel", "n_xseeds"), "pair": ("n_psel",), "cigar": ("n_cigar",), "sam": ("n_recs", "n_md", "n_text")}
# the capacity each count sizes
SIZED = (("out_cap", "n_smem"), ("pos_cap", "n_pos"), ("chain_cap", "n_chains"), ("seed_cap", "n_seeds"), ("reg_cap", "n_regs"),
         ("sel_cap", "n_sel"), ("xreg_cap", "n_xregs"), ("xseed_cap", "n_xseeds"), ("xsel_cap", "n_xsel"), ("psel_cap", "n_psel"),
         ("cigar_cap", "n_cigar"), ("rec_cap", "n_recs"), ("md_cap", "n_md"), ("text_cap", "n_text"))
LIST_COUNT = {"extend": "n_extended", "regs": "n_sel", "rescue": "n_xsel", "pair": "n_psel"}     # of a stage's CIGAR list
COUNT_TENSORS = {"fmi": ("n_out", "n_pos"), "extend": (), "pair": ("count",), "cigar": ("n_cigar",)}  # the others: counts


class Stages:
    """The stages by name (``stages.regs``, ...), behind a ``fmi.DeviceFmi`` that has its suffix-array samples (with the text,
    l_pac and contig_off) or behind a ``mem_chain.DeviceSeedExtension`` that has been queued (`ext`).  skip: the stages left out;
    without "pair" the reads are single (id0 is read_id0, else pair_id0), without "rescue" the paired stage makes the estimate.
    pes: a given estimate.  params: per stage name ("extend": the seed params; "pair" goes to the rescue too).  caps: the
    capacity arguments of all stages in one dict (CAPS, and pos_cap); what is missing takes the stage's default.  sam_input:
    (names, qual, contig_names)."""

    def __init__(self, fmi=None, text=None, l_pac=None, contig_off=None, ext=None, skip=(), id0=0, pes=None, max_occ=500, params=None,
                 caps=None, sam_input=None):
        self.names = [n for n in ORDER if n not in skip]
        self.st = {"fmi": fmi} if ext is None else {"extend": ext}
        self.text, self.l_pac, self.contig_off = text, l_pac, contig_off
        self.id0, self.pes, self.max_occ, self.sam_input = int(id0), pes, max_occ, sam_input
        self.params = {k: v for k, v in (params or {}).items() if v is not None}
        self.caps = dict(caps or {})
        self.params.setdefault("extend", BS.make_seed_params())
        self.pes_in = None                               # what the paired stage takes: read from the rescue once, or `pes`

    def __getattr__(self, name):
        try:
            return self.__dict__["st"][name]
        except KeyError:
            raise AttributeError(name) from None

    def _last(self, *names):
        return self.st[[n for n in names if n in self.names][-1]]

    def _range(self, first, last):
        lo, hi = ORDER.index(first or "fmi"), ORDER.index(last or "sam")
        return [n for n in self.names if lo <= ORDER.index(n) <= hi]

    def make(self, name, stream=None):
        """(Re)builds one stage behind the stages before it, which have been queued on `stream`."""
        p, st = self.params.get(name), self.st
        kw = {k: self.caps[k] for k in CAPS.get(name, ()) if k in self.caps}
        if name == "chain":
            st[name] = MC.DeviceMemChain(st["fmi"], self.l_pac, self.contig_off, p, **kw)
        elif name == "extend":
            st[name] = st["chain"].extension(self.text)
        elif name == "regs":
            st[name] = MR.DeviceMemRegs(st["extend"], p, read_id0=(2 if "pair" in self.names else 1) * self.id0, **kw)
        elif name == "rescue":
            st[name] = MS.DeviceMemRescue(st["regs"], p, self.params.get("pair"), pes=self.pes, **kw)
        elif name == "pair":
            if self.pes_in is None:                      # the one 128-byte copy and synchronisation of the host pointer
                self.pes_in = st["rescue"].pes_host(stream) if "rescue" in self.names else self.pes
            st[name] = MP.DeviceMemPair(self._last("regs", "rescue"), p, pes_in=self.pes_in, **kw)
        elif name == "cigar":
            st[name] = MG.DeviceMemCigar(self._last("extend", "regs", "rescue", "pair").cigar_input, p, **kw)
        elif name == "sam":
            st[name] = SM.DeviceMemSam(self._last("regs", "rescue", "pair"), st["cigar"], *self.sam_input, params=p, **kw)
        return st[name]

    def steps(self, stream=None, first=None, last=None):
        """[(name, callable)] of the stages first..last, all built: what queue() calls, fmi as "smem" and "sal"."""
        out = []
        for name in self._range(first, last):
            s = self.st[name]
            if name == "fmi":
                out += [("smem", lambda s=s: s.run(stream)),
                        ("sal", lambda s=s: s.sal(self.max_occ, pos_cap=self.caps.get("pos_cap"), stream=stream))]
            elif name == "extend":
                out.append((name, lambda s=s: s.run(self.params["extend"], stream)))
            else:
                out.append((name, lambda s=s: s.run(stream)))
        return out

    def queue(self, stream=None, first=None, last=None):
        """Queues the stages first..last on `stream` (a raw hipStream_t handle or None), building those not yet built."""
        for name in self._range(first, last):
            if name not in self.st:
                self.make(name, stream)
            for _, fn in self.steps(stream, name, name):
                fn()
        return self

    def _results(self, name):
        s = self.st[name]
        return (s.results(), s.sal_results()) if name == "fmi" else s.results()

    def check(self):
        """{name: results()} of every stage built, after a synchronisation; a stage whose capacity overflowed raises."""
        return {name: self._results(name) for name in self.names if name in self.st}

    def counts(self, first=None, last=None):
        """The counts the stages first..last left on the device, by the names of COUNTS."""
        out = {}
        for name in self._range(first, last):
            vals = [int(x) for a in COUNT_TENSORS.get(name, ("counts",)) for x in getattr(self.st[name], a).cpu()]
            out.update(zip(COUNTS.get(name, ()), vals))
        return out

    def tighten(self, stream=None, margin=64, first=None, last=None):
        """The sizing pass: stage by stage, queue it with the capacities it has (behind tight stages, so that no default grows
        from a generous one), read its counts, rebuild it at count + margin and queue it again.  The CIGAR stage's direction
        room is the per-record room at the longest extended query and window, times its list's count.  -> the counts, with
        n_extended, lq_max and lt_max of the extension and z_per_record."""
        import ctypes as C
        n = {}
        for name in self._range(first, last):
            if name == "pair":                           # the regions always suffice; the list before it need not
                self.caps["psel_cap"] = self._last("regs", "rescue").regions.cap
            if name == "cigar":
                src = [k for k in LIST_COUNT if k in self.names][-1]
                cp = self.params.setdefault("cigar", MG.make_params())
                n["z_per_record"] = int(MG.lib().gbx_mem_cigar_record_z_bytes(C.byref(cp), n["lq_max"], n["lt_max"]))
                self.caps["z_bytes"] = n[LIST_COUNT[src]] * n["z_per_record"]
            if name != "fmi":
                self.make(name, stream)
            self.queue(stream, name, name)
            N.check(N.lib().gbx_stream_synchronize(stream))
            res = self._results(name)                    # raises when the capacities it has did not suffice
            n.update(self.counts(name, name))
            if name == "extend":
                reg = res[res[:, 2] >= 0]
                n.update(n_extended=len(reg), lq_max=int((reg[:, 3] - reg[:, 2]).max()), lt_max=int((reg[:, 5] - reg[:, 4]).max()))
                continue
            self.caps.update({cap: n[cnt] + margin for cap, cnt in SIZED[1:] if cnt in COUNTS[name]})      # out_cap stays the DeviceFmi's
            if name != "fmi":
                self.make(name, stream)
            self.queue(stream, name, name)
        return n
