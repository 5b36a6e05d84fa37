"""bench.py without and with --full: a plain run does the set-up, the warm-up, the timed steps, --dump-outputs and the line;
the oracle check, the host entry, the drivers end to end and the CPU baseline wait for --full, which leaves what the timed
steps computed as it was."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import has_gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
FULL_ONLY = ("gather_verified", "host_entry", "host_entry_ms", "e2e", "e2e_ms", "cpu_baseline")


def _line(d, *extra):
    r = subprocess.run([sys.executable, BENCH, "--kernel", "bsw", "--size", "3000", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(d)] + list(extra), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
@pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")
def test_plain_run_leaves_the_extra_legs_to_full(tmp_path):
    plain = _line(tmp_path / "plain")
    full = _line(tmp_path / "full", "--full", "--cpu-units", "500")
    for line in (plain, full):
        assert line["metric"] == "bsw_large_gcups" and line["unit"] == "GCUPS" and line["higher_is_better"] is True
        assert line["dtype"] == "int32" and line["steps"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0
    assert not [k for k in FULL_ONLY if k in plain]
    assert not [k for k in FULL_ONLY if k not in full]
    assert "identical" in full["gather_verified"] and "DIFFER" not in full["gather_verified"]
    assert full["host_entry"]["same_as_device_entry"] is True and "identical to" in full["cpu_baseline"]["verified"]
    names = sorted(os.path.basename(p) for p in glob.glob(str(tmp_path / "plain" / "*.npy")))
    assert names == ["bsw_pair.npy", "bsw_result.npy"]
    for nm in names:
        assert np.array_equal(np.load(str(tmp_path / "plain" / nm)), np.load(str(tmp_path / "full" / nm)))
