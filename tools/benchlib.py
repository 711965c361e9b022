"""The measuring method of the tools/*_bench.py scripts, once: plain functions a timing tool is written on top of.

A tool keeps its workloads, buffers, version list, derived figures and result layout; what decides whether its numbers can be
compared with those in profiles/ lives here:
  parser / start / finish   the common options, the commit stamp, the JSON line and the --out file
  bind / option             ttm_last_kernel and ttm_set_option of the loaded library
  warm_up                   every version in order: its option pinned, some launches, the kernel that ran
  keep_busy                 a second of untimed launches (the chip holds its clock only while it is kept busy: bench.py)
  time_rounds               the versions alternated round by round, settle launches, then a clock around a batch
  summarise / report        median, min, max and spread over the rounds; the one-line console summary
A version is (name, option value or None, fn).  `pin` is None (the tool has no option, or the library does not know it) or a
callable taking the value; None as a version's value stands for -1, the library's own plan, and -1 is what is left behind.
Times come from a clock object (start(), stop() -> ms, sync()); the default puts two HIP events around the batch.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys


class EventClock:
    """Two HIP events on the current stream around what runs between start() and stop(); stop() synchronises."""

    def __init__(self):
        import torch
        self.cuda = torch.cuda

    def start(self):
        self.a, self.b = self.cuda.Event(enable_timing=True), self.cuda.Event(enable_timing=True)
        self.a.record()

    def stop(self):
        self.b.record()
        self.cuda.synchronize()
        return self.a.elapsed_time(self.b)

    def sync(self):
        self.cuda.synchronize()


def parser(doc, launches, workloads=None):
    ap = argparse.ArgumentParser(description=doc, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help='the repository tree whose package is timed')
    ap.add_argument('--label', default='')
    ap.add_argument('--out', default='')
    ap.add_argument('--launches', type=int, default=launches)
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--rows', type=int, default=0, help='rows instead of the workload\'s own N (rehearsals)')
    ap.add_argument('--commit', default='', help='what to record as the commit when the tree is not a git checkout')
    if workloads is not None:
        ap.add_argument('--workloads', default=workloads)
    return ap


def start(args, launches_key='launches_per_version'):
    """args.root on sys.path, torch and bench imported; (bench, res) with the head of the result: label, launches, rounds, commit."""
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import torch  # noqa: F401  (its HIP runtime before the library's)
    import bench
    res = {'label': args.label, launches_key: args.launches, 'rounds': args.rounds}
    try:
        res['commit'] = subprocess.run(['git', '-C', root, 'rev-parse', '--short', 'HEAD'], capture_output=True, text=True).stdout.strip()
    except OSError:
        res['commit'] = ''
    res['commit'] = res['commit'] or args.commit
    return bench, res


def per_round(args):
    return max(1, args.launches // args.rounds)


def bind(lib):
    """Declares ttm_set_option / ttm_last_kernel; returns a callable that names the kernel of the last launch."""
    import ctypes
    lib.ttm_set_option.argtypes = [ctypes.c_char_p, ctypes.c_int32]
    lib.ttm_last_kernel.restype = ctypes.c_char_p
    return lambda: lib.ttm_last_kernel().decode()


def option(lib, name, probe=False):
    """The pin of one launch option.  probe: None where the library does not know the option (an older tree under --root)."""
    key = name.encode()
    if probe and lib.ttm_set_option(key, -1) != 0:
        return None
    return lambda value: lib.ttm_set_option(key, value)


def _pin(pin, opt):
    if pin is not None:
        pin(-1 if opt is None else opt)


def warm_up(versions, pin, launches, kernel, after=None, clock=None):
    """First launches of every version (tables, code objects), the kernel each took; after(name, info[name]) adds a tool's own checks."""
    clock = clock or EventClock()
    info = {}
    for name, opt, fn in versions:
        _pin(pin, opt)
        for _ in range(launches):
            fn()
        clock.sync()
        info[name] = {'kernel': kernel(), 'ms_rounds': []}
        if after is not None:
            after(name, info[name])
    return info


def keep_busy(fn, batch, ms=1000.0, clock=None):
    """Batches of fn until the clock has seen `ms` of them: nothing is timed on a chip that has been idle."""
    clock = clock or EventClock()
    busy = 0.0
    while busy < ms:
        clock.start()
        for _ in range(batch):
            fn()
        busy += clock.stop()


def time_rounds(versions, info, pin, rounds, per, settle, clock=None):
    """`rounds` times over the versions in order: option pinned, `settle` untimed launches, the clock around `per` launches (one int, or
    a dict by version name); the mean launch time of the batch goes to info[name]['ms_rounds'].  The option is -1 afterwards."""
    clock = clock or EventClock()
    for _ in range(rounds):
        for name, opt, fn in versions:
            n = per[name] if isinstance(per, dict) else per
            _pin(pin, opt)
            for _ in range(settle):
                fn()
            clock.start()
            for _ in range(n):
                fn()
            info[name]['ms_rounds'].append(clock.stop() / n)
    _pin(pin, -1)


def summarise(v, gbytes=None, roof=None):
    """Median, min, max and relative spread of v['ms_rounds']; with gbytes, the share of the `roof` GB/s the median moves them at."""
    r = v['ms_rounds']
    v['ms'] = float(statistics.median(r))
    v['ms_min'], v['ms_max'] = float(min(r)), float(max(r))
    v['spread_rel'] = (v['ms_max'] - v['ms_min']) / v['ms']
    if gbytes is not None:
        v['hbm_frac_on_algorithmic_bytes'] = gbytes / (v['ms'] * 1e-3) / roof


def report(key, info, *more):
    print(key, json.dumps({k: (v['kernel'], round(v['ms'], 4), round(v['ms_min'], 4), round(v['ms_max'], 4)) for k, v in info.items()}),
          *more, flush=True)


def finish(res, out):
    print(json.dumps(res))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)) or '.', exist_ok=True)
        with open(out, 'w') as f:
            json.dump(res, f, indent=1)
