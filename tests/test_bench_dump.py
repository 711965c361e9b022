"""bench.py --dump-outputs: the samples of the timed step's outputs it writes are the same in every run and fit 64 MB;
a plain run (no --full) writes them and prints the headline line alone."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_sample_is_fixed_sorted_and_bounded():
    for N, rows in ((1000000, 80), (1000000, 4), (500000, 8), (70001, 80), (1000, 80)):
        a, b = bench.dump_sample_index(N, rows), bench.dump_sample_index(N, rows)
        assert np.array_equal(a, b)
        assert a[0] >= 0 and a[-1] < N and np.all(np.diff(a) > 0)
        assert a.size * rows * 8 <= 64 << 20
    assert np.array_equal(bench.dump_sample_index(1000, 80), np.arange(1000))


@pytest.mark.gpu
def test_plain_run_prints_the_headline_line_and_writes_the_dump(tmp_path):
    N = 70001
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '3', '--warmup', '1', '--n', str(N),
                          '--prewarm-seconds', '0', '--dump-outputs', str(tmp_path)],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, res.stdout[-2000:]
    js = json.loads(lines[0])
    D, d = js['config']['D'], js['config']['columns']
    assert js['unit'] == 'map-evals/s' and js['dtype'] == 'f64' and js['higher_is_better'] is True
    assert js['steps'] == 3 and js['warmup'] == 1 and js['ms_per_step'] > 0
    assert js['value'] == pytest.approx(N * D * 1e3 / js['ms_per_step'], rel=1e-12)
    # what only --full measures or checks stays out of a plain run
    assert not {'roofline', 'kernel_timing', 'cold_ms_per_step', 'uncached_ms_per_step', 'roundtrip_max_abs_err',
                'optimize_s', 'api_map_ms', 'other_configs', 'cpu_baseline'} & set(js)
    idx = bench.dump_sample_index(N, D + d)
    Z, X = np.load(tmp_path / 'forward_Z.npy'), np.load(tmp_path / 'inverse_X.npy')
    assert Z.shape == (idx.size, D) and X.shape == (idx.size, d)
    assert Z.dtype == X.dtype == np.float64 and np.all(np.isfinite(Z)) and np.all(np.isfinite(X))
