"""bench.py's plain run and --dump-outputs (run with -m gpu): the plain line carries none of the --full extras, and the dump is a
fixed sample of the last timed step's outputs -- float32 / float64 only, under 64 MB, the same in two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--frames", "64", "--steps", "3", "--warmup", "1", *args],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_plain_run_dumps_a_reproducible_sample_of_the_last_step(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    d = _bench("--dump-outputs", str(a))
    _bench("--dump-outputs", str(b))
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["cpu_baseline"] is None and d["config"]["bit_error_rate_frame0"] is None
    assert d["roofline"]["measured_copy_GBs"] is None and d["roofline"]["package_power_w_and_sclk_mhz_under_load"] is None
    names = sorted(os.listdir(a))
    assert names == ["bits.npy", "bits_index.npy", "eq_symbols.npy", "eq_symbols_index.npy"]
    assert sum(os.path.getsize(a / n) for n in names) <= 64 << 20
    out = {n[:-4]: np.load(a / n) for n in names}
    for n in out:
        assert out[n].dtype in (np.float32, np.float64), n
        assert np.array_equal(out[n], np.load(b / (n + ".npy"))), n
    eq, rows = out["eq_symbols"], out["eq_symbols_index"]
    assert eq.shape[1:] == (180, 1200, 2) and eq.shape[0] == len(rows) >= 1 and np.isfinite(eq).all()
    assert np.all(np.diff(rows) > 0) and rows[-1] < 64
    bits = out["bits"]                                   # 64 frames of packed 16-QAM bits fit the budget whole
    assert bits.shape == (64, 180 * 1200 * 4 // 8) and np.array_equal(out["bits_index"], np.arange(64))
    assert np.array_equal(bits, np.round(bits)) and bits.min() >= 0 and bits.max() <= 255
