"""The timing tools on top of tools/benchlib.py still run and still write what they wrote: each of the six in a fresh child process on the
smallest arguments that take the planned kernels (65 536 rows: from there band_forward_gate / rt_shape_gate let a call onto the band
kernels), the tree of keys of its JSON line against the one its version before benchlib wrote for the same arguments."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ['--rows', '65536', '--launches', '4', '--rounds', '2']


def keys(*leaves, **subtrees):
    return {**dict.fromkeys(leaves), **subtrees}


HEAD = ('label', 'launches_per_version', 'rounds', 'commit')
V = ('kernel', 'ms_rounds', 'ms', 'ms_min', 'ms_max', 'spread_rel')
HBM = V + ('hbm_frac_on_algorithmic_bytes',)
NEWTON = HBM + ('round_trip_max', 'trial_points_max_per_component', 'fp64_frac_upper_bound')
BISECT = ('kernel_rows_1_on', 'round_trip_max_rows_1_on', 'midpoints_max_per_component') + V[1:]
FILL = V + ('launches_per_round', 'written_gbytes', 'written_GBs', 'copy_peak_frac', 'counted_fp64_TFLOPs', 'fp64_peak_frac')
HOST = keys('ms', 'ms_min', 'ms_max')
STEP = HBM + ('algorithmic_gbytes',)

# tool: (its arguments beside SMALL, the key tree of its JSON line - lists are leaves -, the child's time limit in seconds).
# The trees are those of the tools as they were before tools/benchlib.py, run with these arguments on an MI355X; the time limits end a
# hang and gate no speed: five times the wall time of that run (map build and the one-second busy phase: they vary with the machine's
# load), rounded up to a multiple of 10 s.
TOOLS = {
    'score_bench.py': (['--workloads', 'C2b'], keys(*HEAD, workloads=keys(C2b=keys(
        'N', 'D', 'd', 'algorithmic_gbytes', 'band_over_forward_time', 'generic_over_band_time',
        versions=keys(band=keys(*HBM), band_std=keys(*HBM), generic=keys(*HBM, 'max_rel_diff_to_band'), forward=keys(*HBM))))),
        30),                                                                   # measured: 4.68 s
    'newton_bench.py': (['--workloads', 'C2b'], keys(*HEAD, workloads=keys(C2b=keys(
        'N', 'D', 'algorithmic_gbytes', 'newton_over_generic', 'newton_over_table_time',
        versions=keys(newton=keys(*NEWTON), generic=keys(*NEWTON), table=keys(*HBM, 'round_trip_max'))))),
        30),                                                                   # measured: 4.68 s
    'bisect_bench.py': (['--workloads', 'C2b'], keys(*HEAD, workloads=keys(C2b=keys(
        'N', 'D', 'generic_over_bisect', 'bisect_over_newton', 'bisect_over_table',
        versions=keys(bisect=keys(*BISECT, 'share_bit_identical_to_generic', 'max_abs_difference_to_generic'), generic=keys(*BISECT),
                      newton=keys(*V, 'round_trip_max_rows_1_on'), table=keys(*V, 'round_trip_max_rows_1_on'))))),
        30),                                                                   # measured: 4.43 s
    'sample_bench.py': (['--workloads', 'C2b'], keys(*HEAD, 'flop_per_pair', 'copy_peak_GBs', 'fp64_peak_TFLOPs', workloads=keys(C2b=keys(
        'N', 'D', 'd', 'fill_over_inverse_device_time', 'sample_device_over_inverse_device_time', 'sample_over_inverse_map_time',
        device=keys(fill=keys(*FILL), fill_odd=keys(*FILL), inverse_device=keys(*V, 'launches_per_round'),
                    sample_device=keys(*V, 'launches_per_round', 'equals_inverse_device_of_the_fill')),
        host=keys(sample=HOST, inverse_map=HOST)))),
        30),                                                                   # measured: 4.34 s
    'logdensity_bench.py': (['--workloads', 'C2a'], keys(*HEAD, workloads=keys(C2a=keys(
        'N', 'D', 'd', 'Q', 'logdensity_over_forward_time', 'logdensity_over_forward_generic_time', 'logp_only_over_forward_generic_time',
        'finite_difference_passes', 'finite_difference_step_ms', 'finite_difference_step_generic_ms',
        'finite_differences_over_logdensity_time', 'finite_differences_generic_over_logdensity_time',
        versions=keys(logdensity=keys(*V), logp_only=keys(*V), forward=keys(*V, 'max_rel_diff_of_logp'),
                      forward_generic=keys(*V, 'max_rel_diff_of_logp'))))),
        30),                                                                   # measured: 4.05 s
    'band_linear_bench.py': (['--maps', 'linear'], keys('label', 'launches_per_step', 'rounds', 'commit', maps=keys(linear=keys(
        'N', 'D', 'u_p_lag', 'u_h_cls', 'u_h_ng',
        steps=keys(forward=keys(*STEP), density=keys(*STEP), logdet=keys(*STEP), sumsq=keys(*STEP), table=keys(*STEP, 'round_trip_max'),
                   newton=keys(*STEP, 'round_trip_max', 'trial_points_max_per_component'))))),
        20),                                                                   # measured: 3.31 s
}


def tree(x):
    return {k: tree(v) for k, v in x.items()} if isinstance(x, dict) else None


def leaves(x, name):
    """every value stored under the key `name`, at any depth"""
    if isinstance(x, dict):
        for k, v in x.items():
            if k == name:
                yield v
            else:
                yield from leaves(v, name)


@pytest.mark.gpu
@pytest.mark.parametrize('tool', sorted(TOOLS))
def test_tool_runs_and_writes_what_it_wrote(tool, tmp_path):
    extra, schema, limit = TOOLS[tool]
    out = tmp_path / 'result.json'
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', tool)] + SMALL + extra + ['--label', 'small', '--out', str(out)],
                         capture_output=True, text=True, timeout=limit, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    js = json.loads(res.stdout.splitlines()[-1])
    assert tree(js) == schema
    assert js['label'] == 'small' and js['rounds'] == 2 and json.loads(out.read_text()) == js
    ms, rounds = list(leaves(js, 'ms')), list(leaves(js, 'ms_rounds'))
    names = list(leaves(js, 'kernel')) + list(leaves(js, 'kernel_rows_1_on'))
    assert len(ms) >= 3 and all(t > 0 for t in ms)
    assert len(rounds) >= 3 and all(len(r) == 2 for r in rounds)
    assert len(names) == len(rounds) and all(isinstance(k, str) and k for k in names)
    assert [n for n in leaves(js, 'N')] == [65536]
