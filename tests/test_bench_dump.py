"""bench.py --dump-outputs: the samples of the timed step's outputs it writes are the same in every run and fit 64 MB."""
import numpy as np

import bench


def test_dump_sample_is_fixed_sorted_and_bounded():
    for N, rows in ((1000000, 80), (1000000, 4), (500000, 8), (70001, 80), (1000, 80)):
        a, b = bench.dump_sample_index(N, rows), bench.dump_sample_index(N, rows)
        assert np.array_equal(a, b)
        assert a[0] >= 0 and a[-1] < N and np.all(np.diff(a) > 0)
        assert a.size * rows * 8 <= 64 << 20
    assert np.array_equal(bench.dump_sample_index(1000, 80), np.arange(1000))
