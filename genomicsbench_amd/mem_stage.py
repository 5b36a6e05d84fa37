"""What flows between the bwa-mem stage classes (mem_chain, mem_regs, mem_rescue, mem_pair, mem_cigar, mem_sam), said once.  Every
stage exposes its outputs as these records and reads its inputs from the records of the stage it is given: ``batch`` (all),
``seeds`` (extension, regs, rescue), ``regions`` and ``pairs`` (regs, rescue, pair; ``pairs`` is None but behind the paired stage)
and ``cigar_input`` (extension, regs, rescue, pair).  The tensors are the stages' own; a record copies nothing.
``mem_pipeline.Stages`` queues the stages.
"""
from typing import Any, NamedTuple


class Batch(NamedTuple):
    """The reads and the reference as every stage behind the extension needs them; ``mem_chain.DeviceSeedExtension`` builds it
    and every later stage carries the same object on."""
    device: Any
    n_reads: int
    qer: Any                 # uint8 tensor: the reads' arena, padded
    qer_bytes: int
    read_off: Any            # int64[n_reads]
    read_len: Any            # int32[n_reads]
    ref: Any                 # uint8 tensor: the 2 L-byte text, padded
    ref_bytes: int
    l_pac: int
    n_contigs: int
    contig_off: Any          # int64[n_contigs + 1]


class Regions(NamedTuple):
    """A region list: uint8 tensor of `cap` REG_DTYPE records, the reads' offsets into it, and its count on the device."""
    regs: Any
    reg_off: Any             # int64[n_reads + 1]
    count: Any               # int64[1], a view: count.data_ptr() is what the entries take
    cap: int
    read_id0: int


class Seeds(NamedTuple):
    """The seed records the regions' `seed` fields index: uint8 tensor of `cap` SEED_DTYPE records, and l_rep per read."""
    seeds: Any
    cap: int
    l_rep: Any               # int32[n_reads]


class CigarList(NamedTuple):
    """What ``mem_cigar.DeviceMemCigar`` aligns: n (seed, extension result) records, the tail being no records."""
    batch: Batch
    seeds: Any               # uint8 tensor of n SEED_DTYPE records
    res: Any                 # int32[n, 8]
    n: int
