"""tools/benchlib.py, the measuring method of the tools/*_bench.py scripts: its statistics, the order in which it pins options, launches,
reads kernel names and takes times (a fake clock and recording stand-ins: no GPU), its common options and the commit rule."""
import argparse
import os
import sys

import pytest

from tools import benchlib


def test_summarise_odd_and_even_number_of_rounds():
    v = {'ms_rounds': [0.2, 0.1, 0.4]}
    benchlib.summarise(v)
    assert v['ms'] == 0.2 and v['ms_min'] == 0.1 and v['ms_max'] == 0.4
    assert v['spread_rel'] == pytest.approx(1.5, rel=1e-12)
    assert 'hbm_frac_on_algorithmic_bytes' not in v and v['ms_rounds'] == [0.2, 0.1, 0.4]
    v = {'ms_rounds': [0.1, 0.2, 0.3, 0.4]}
    benchlib.summarise(v, gbytes=8.0, roof=8000.0)
    assert v['ms'] == 0.25 and v['ms_min'] == 0.1 and v['ms_max'] == 0.4
    assert v['spread_rel'] == pytest.approx(1.2, rel=1e-12)
    assert v['hbm_frac_on_algorithmic_bytes'] == pytest.approx(8.0 / 0.25e-3 / 8000.0, rel=1e-12) == pytest.approx(4.0, rel=1e-12)


class FakeClock:
    """Every stop() reports `span` ms more than the one before it; what happens goes to the shared log."""

    def __init__(self, log, span=300.0):
        self.log, self.span, self.stops = log, span, 0

    def start(self):
        self.log.append('start')

    def stop(self):
        self.log.append('stop')
        self.stops += 1
        return self.span * self.stops

    def sync(self):
        self.log.append('sync')


def test_order_of_pins_launches_and_times():
    log = []
    clock = FakeClock(log)

    def version(name, opt):
        return (name, opt, lambda: log.append(name))

    def kernel():
        log.append('kernel')
        return 'k_%d' % log.count('kernel')

    def pin(value):
        log.append(('pin', value))

    versions = [version('A', 1), version('B', 0), version('C', None)]
    seen = []
    info = benchlib.warm_up(versions, pin, 3, kernel, after=lambda name, v: seen.append((name, dict(v))), clock=clock)
    # (a version without a value of its own runs on the library's plan, -1: never on what the version before it left pinned)
    assert log == [('pin', 1), 'A', 'A', 'A', 'sync', 'kernel', ('pin', 0), 'B', 'B', 'B', 'sync', 'kernel', ('pin', -1), 'C', 'C', 'C', 'sync', 'kernel']
    assert seen == [('A', {'kernel': 'k_1', 'ms_rounds': []}), ('B', {'kernel': 'k_2', 'ms_rounds': []}), ('C', {'kernel': 'k_3', 'ms_rounds': []})]
    assert list(info) == ['A', 'B', 'C'] and all(info[k] == v for k, v in seen)

    del log[:]
    benchlib.keep_busy(versions[0][2], 2, clock=clock)               # 300 + 600 < 1000 <= 300 + 600 + 900: three batches of the first version
    assert log == ['start', 'A', 'A', 'stop'] * 3

    del log[:]
    per = {'A': 3, 'B': 1, 'C': 2}
    benchlib.time_rounds(versions, info, pin, 2, per, 2, clock=clock)
    one = []
    for name, opt in (('A', 1), ('B', 0), ('C', -1)):
        one += [('pin', opt)] + [name] * 2 + ['start'] + [name] * per[name] + ['stop']
    assert log == one + one + [('pin', -1)]
    # stops 4..9 of the clock, in the order A B C A B C
    assert info['A']['ms_rounds'] == [1200.0 / 3, 2100.0 / 3]
    assert info['B']['ms_rounds'] == [1500.0 / 1, 2400.0 / 1]
    assert info['C']['ms_rounds'] == [1800.0 / 2, 2700.0 / 2]


def test_one_batch_size_for_all_and_no_option():
    log = []
    clock = FakeClock(log, span=1000.0)
    versions = [('x', None, lambda: log.append('x')), ('y', None, lambda: log.append('y'))]
    info = benchlib.warm_up(versions, None, 1, lambda: 'k', clock=clock)
    benchlib.keep_busy(versions[0][2], 4, clock=clock)
    benchlib.time_rounds(versions, info, None, 1, 2, 0, clock=clock)
    assert log == ['x', 'sync', 'y', 'sync', 'start', 'x', 'x', 'x', 'x', 'stop', 'start', 'x', 'x', 'stop', 'start', 'y', 'y', 'stop']
    assert info == {'x': {'kernel': 'k', 'ms_rounds': [1000.0]}, 'y': {'kernel': 'k', 'ms_rounds': [1500.0]}}


def test_probed_option_is_none_where_the_library_does_not_know_it():
    class Lib:
        calls = []

        def ttm_set_option(self, key, value):
            self.calls.append((key, value))
            return 0 if key == b'band_newton' else -1

    lib = Lib()
    assert benchlib.option(lib, 'band_bisect', probe=True) is None
    pin = benchlib.option(lib, 'band_newton', probe=True)
    pin(0)
    assert lib.calls == [(b'band_bisect', -1), (b'band_newton', -1), (b'band_newton', 0)]


def test_parser_has_rows_and_root_for_every_tool():
    ap = benchlib.parser('doc', 40)                                   # (a tool that had neither, and no --workloads)
    args = ap.parse_args([])
    assert args.rows == 0 and args.launches == 40 and args.rounds == 10 and args.label == '' and args.out == '' and args.commit == ''
    assert os.path.isfile(os.path.join(args.root, 'bench.py')) and not hasattr(args, 'workloads')
    args = ap.parse_args(['--rows', '65536', '--root', '/somewhere/else', '--launches', '4', '--rounds', '2'])
    assert args.rows == 65536 and args.root == '/somewhere/else' and args.launches == 4 and args.rounds == 2
    ap = benchlib.parser('doc', 200, 'C5,C2b')
    ap.add_argument('--host-reps', type=int, default=7)
    assert ap.parse_args([]).workloads == 'C5,C2b' and ap.parse_args(['--workloads', 'C3']).workloads == 'C3'
    assert benchlib.per_round(argparse.Namespace(launches=200, rounds=10)) == 20
    assert benchlib.per_round(argparse.Namespace(launches=4, rounds=10)) == 1


def test_start_stamps_the_commit_it_is_given_outside_a_checkout(tmp_path, monkeypatch):
    (tmp_path / 'bench.py').write_text('HBM_PEAK_GBS = 1.0\n')
    monkeypatch.delitem(sys.modules, 'bench', raising=False)
    monkeypatch.setattr(sys, 'path', list(sys.path))
    monkeypatch.setenv('GIT_CEILING_DIRECTORIES', str(tmp_path.parent))      # (a temporary directory inside some checkout stays outside it)
    args = benchlib.parser('doc', 50).parse_args(['--root', str(tmp_path), '--commit', 'abc', '--label', 'here', '--rounds', '3'])
    bench, res = benchlib.start(args)
    assert bench.HBM_PEAK_GBS == 1.0 and sys.path[0] == str(tmp_path)
    assert res == {'label': 'here', 'launches_per_version': 50, 'rounds': 3, 'commit': 'abc'}
    _, res = benchlib.start(args, 'launches_per_step')
    assert res == {'label': 'here', 'launches_per_step': 50, 'rounds': 3, 'commit': 'abc'}
    sys.modules.pop('bench', None)
