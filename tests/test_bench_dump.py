"""bench.py --dump-outputs: what the timed steps returned, as .npy files that two builds can be compared on.

On CPU the oracle's results, laid out as the device entries leave them, go through each kernel's dump and must come back
unit for unit; on the GPU a real bench run's dump must equal the oracle on the units it kept, and two runs with the same
arguments must write the same arrays."""
import argparse
import glob
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import has_gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
SIZES = {"bsw": 3000, "chain": 40, "phmm": 30, "poa": 6, "abea": 5, "fmi": 3000}
FMI_GENOME = 1 << 20


def _bench():
    spec = importlib.util.spec_from_file_location("bench_dump_mod", BENCH)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _inputs(m, kind):
    """The bench's own inputs of a `--kernel kind --size SIZES[kind]` run, and the oracle's results on them."""
    from oracle import oracle_py as O
    saved = os.environ.get("GBX_FMI_GENOME")
    os.environ["GBX_FMI_GENOME"] = str(FMI_GENOME)
    try:
        w = m.WORKLOADS[kind](argparse.Namespace(size=SIZES[kind]))
        host = w.generate(0, w.n)
    finally:
        if saved is None:
            del os.environ["GBX_FMI_GENOME"]
        else:
            os.environ["GBX_FMI_GENOME"] = saved
    if kind == "bsw":
        want = O.bsw_oracle(w.params, host, 4)
    elif kind == "chain":
        want = np.stack(O.chain_oracle(*host, nthreads=4), axis=1)
    elif kind == "phmm":
        want = O.phmm_oracle(host, 4)
    elif kind == "poa":
        want = O.poa_oracle(w.params, host, 4)
    elif kind == "abea":
        want = O.abea_oracle(host, 4)
    else:
        from genomicsbench_amd.fmi import build_index
        want = O.fmi_oracle(build_index(w.genome_codes()).host(), host, nthreads=4)
    return w, host, want


def _device_layout(kind, host, want):
    """The oracle's results as the bench gathers them from the device (bench.py *Work.output_tensor)."""
    import torch
    if kind in ("bsw", "chain", "phmm"):
        return torch.from_numpy(np.ascontiguousarray(want))
    if kind == "poa":
        stride = host.default_stride
        rec = np.full((len(want), 8 + stride), 0xAB, dtype=np.uint8)       # bytes past a consensus are not part of it
        head = np.zeros((len(want), 2), dtype=np.int32)
        head[:, 1] = [len(s) for s in want]
        rec[:, :8] = head.view(np.uint8)
        for k, s in enumerate(want):
            rec[k, 8:8 + len(s)] = np.frombuffer(s.encode(), dtype=np.uint8)
        return torch.from_numpy(rec)
    if kind == "abea":
        wo, wn = want
        flat = np.stack([wo["ref_pos"], wo["read_pos"]], axis=1).astype(np.int32)
        for r in range(host.n_reads):                                       # slots past a read's pairs are not part of it
            a = 2 * int(host.event_off[r])
            flat[a + int(wn[r]):2 * int(host.event_off[r + 1])] = -7
        return torch.from_numpy(np.concatenate([flat.reshape(-1), wn.astype(np.int32)]))
    wo, woff = want
    return torch.from_numpy(np.concatenate([np.array([len(wo)], np.int64).view(np.uint8), woff.astype(np.int64).view(np.uint8),
                                            np.ascontiguousarray(wo).view(np.uint8)]))


def _check(kind, host, want, d):
    """Every array of the dump in `d` against the oracle's results on the units it names."""
    def load(name):
        a = np.load(os.path.join(d, "%s_%s.npy" % (kind, name)))
        assert a.dtype in (np.float32, np.float64)
        return a
    if kind in ("bsw", "chain"):
        idx = load("pair" if kind == "bsw" else "anchor").astype(np.int64)
        assert len(idx) and np.array_equal(load("result"), want[idx])
    elif kind == "phmm":
        idx, got = load("pair").astype(np.int64), load("log10_likelihood")
        w = want[idx]
        fin = np.isfinite(w)
        assert len(idx) and np.array_equal(np.isfinite(got), fin)
        assert np.all(np.abs(got[fin] - w[fin]) <= 1e-5 * np.maximum(1.0, np.abs(w[fin])))
    elif kind == "poa":
        idx = load("window").astype(np.int64)
        assert len(idx) and not load("status").any()
        lens, cons = load("consensus_len").astype(np.int64), load("consensus").astype(np.uint8)
        assert list(lens) == [len(want[w]) for w in idx]
        assert cons.tobytes().decode() == "".join(want[w] for w in idx)
    elif kind == "abea":
        wo, wn = want
        idx, n, pairs = load("read").astype(np.int64), load("n_pairs").astype(np.int64), load("pairs")
        assert len(idx) and np.array_equal(n, wn[idx])
        exp = [np.stack([wo["ref_pos"][a:a + c], wo["read_pos"][a:a + c]], axis=1)
               for a, c in ((2 * int(host.event_off[r]), int(wn[r])) for r in idx)]
        assert np.array_equal(pairs, np.concatenate(exp))
    else:
        wo, woff = want
        idx, n, smems = load("read").astype(np.int64), load("n_smems").astype(np.int64), load("smems")
        assert len(idx) and np.array_equal(n, np.diff(woff)[idx])
        rows = np.stack([wo[f].astype(np.int64) for f in ("rid", "m", "n", "k", "l", "s")], axis=1)
        assert np.array_equal(smems, np.concatenate([rows[woff[r]:woff[r + 1]] for r in idx]))
    return sum(os.path.getsize(p) for p in glob.glob(os.path.join(d, kind + "_*.npy")))


def test_dump_sample_keeps_everything_that_fits_and_a_fixed_sample_otherwise():
    m = _bench()
    assert np.array_equal(m._dump_sample(np.full(100, 7), 8 * 700), np.arange(100))
    sizes = np.arange(1, 50001) % 97 + 1
    a, b = m._dump_sample(sizes, 1 << 20), m._dump_sample(sizes, 1 << 20)
    assert np.array_equal(a, b) and 0 < len(a) < len(sizes)
    assert np.all(np.diff(a) > 0) and 8 * sizes[a].sum() <= 1 << 20
    assert len(m._dump_sample(np.full(10, 1000), 8)) == 1


@pytest.mark.parametrize("kind", sorted(SIZES))
def test_dump_of_the_device_layout_returns_the_oracle_unit_for_unit(kind, tmp_path):
    """A small budget forces the sample; the written units must be exactly the oracle's (pad bytes and unused slots of
    the device layout excluded)."""
    m = _bench()
    w, host, want = _inputs(m, kind)
    n = w.n_units(host)
    arrays = w.dump_arrays([_device_layout(kind, host, want)], [(host, 0, n)], 4096)
    nbytes = m._write_dump(str(tmp_path), kind, arrays)
    units = len(next(iter(arrays.values())))
    assert units == 1 or (1 < units and nbytes <= 4096)            # at least one unit is always written
    _check(kind, host, want, str(tmp_path))
    full = w.dump_arrays([_device_layout(kind, host, want)], [(host, 0, n)], 1 << 30)
    assert len(next(iter(full.values()))) == (len(want) if kind in ("bsw", "chain", "phmm", "poa") else n)


def test_dump_budget_of_a_whole_run_stays_under_64_mb():
    m = _bench()
    assert set(m.DUMP_SHARE) == set(m.WORKLOADS) and sum(m.DUMP_SHARE.values()) <= 1.0
    assert m.DUMP_BYTES + 32 * 128 <= 64 << 20                     # + the .npy headers


def _run_bench(kind, d, steps=2):
    env = dict(os.environ, GBX_FMI_GENOME=str(FMI_GENOME))
    r = subprocess.run([sys.executable, BENCH, "--kernel", kind, "--size", str(SIZES[kind]), "--steps", str(steps), "--warmup", "1",
                        "--no-cpu", "--dump-outputs", str(d)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r


@pytest.mark.gpu
@pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")
@pytest.mark.parametrize("kind", sorted(SIZES))
def test_bench_dump_equals_the_oracle(kind, tmp_path):
    import json
    r = _run_bench(kind, tmp_path / "d", steps=3)
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    m = _bench()
    w, host, want = _inputs(m, kind)
    assert 0 < _check(kind, host, want, str(tmp_path / "d")) <= 64 << 20


@pytest.mark.gpu
@pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")
def test_two_bench_runs_dump_the_same_arrays(tmp_path):
    for d in ("a", "b"):
        _run_bench("bsw", tmp_path / d)
    names = sorted(os.path.basename(p) for p in glob.glob(str(tmp_path / "a" / "*.npy")))
    assert names == ["bsw_pair.npy", "bsw_result.npy"]
    assert names == sorted(os.path.basename(p) for p in glob.glob(str(tmp_path / "b" / "*.npy")))
    for nm in names:
        assert np.array_equal(np.load(str(tmp_path / "a" / nm)), np.load(str(tmp_path / "b" / nm)))
