"""Hardware counters of the score kernel beside the forward map at C5 (d = 40, N = 1e6): what `profiles/score_pmc_C5.json` holds.

Two roles.  Under the profiler, as the program that is profiled - five launches each of ttm_score with g_scale and ld_affine,
ttm_score without them, and ttm_forward on the same buffers, in that order:

    rocprofv3 --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_ACTIVE_INST_VALU -d OUT/a --output-format csv -- python tools/score_pmc.py run
    rocprofv3 --pmc SQ_INSTS_LDS SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT SQ_WAIT_INST_LDS -d OUT/b --output-format csv -- python tools/score_pmc.py run

(counters alone: no tracing beside them; one pass of four counters per run).  Afterwards, anywhere:

    python tools/score_pmc.py summarise OUT profiles/score_pmc_C5.json

averages every counter over the launches of a kernel; the launches of k_band_score alternate raw / standardised in dispatch order.
"""
import collections
import csv
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run():
    sys.path.insert(0, ROOT)
    import torch
    import bench
    tm, X, cfg = bench.build_map('C5', 0)
    N, D = tm._N, tm.D
    coef = tm._pack_coeffs()
    std, mean = np.asarray(tm.X_std, float)[:D], np.asarray(tm.X_mean, float)[:D]
    gs = tm._to_dev(1.0 / std)
    af = tm._to_dev(np.ascontiguousarray(np.column_stack((std, mean))))
    G = tm._cols(D, N)
    for _ in range(5):
        tm.score_device(tm._Xs, N, coef=coef, G=G, g_scale=gs, ld_affine=af)
        tm.score_device(tm._Xs, N, coef=coef, G=G)
        tm.forward_device(tm._Xs, N, coef=coef, Z=G)
    torch.cuda.synchronize()


def summarise(src, dst):
    res = collections.defaultdict(lambda: collections.defaultdict(list))
    for f in glob.glob(os.path.join(src, '**', '*counter_collection.csv'), recursive=True):
        for r in csv.DictReader(open(f)):
            k = r['Kernel_Name']
            if 'k_band_score' in k or 'k_band_forward' in k:
                res['k_band_score' if 'score' in k else 'k_band_forward'][r['Counter_Name']].append((int(r['Dispatch_Id']), float(r['Counter_Value'])))
    out = {}
    for name, counters in res.items():
        for cn, v in counters.items():
            v.sort()
            if name == 'k_band_score':
                out.setdefault('k_band_score (g_scale, ld_affine)', {})[cn] = float(np.mean([x for i, (_, x) in enumerate(v) if i % 2 == 0]))
                out.setdefault('k_band_score (standardised)', {})[cn] = float(np.mean([x for i, (_, x) in enumerate(v) if i % 2 == 1]))
            else:
                out.setdefault(name, {})[cn] = float(np.mean([x for _, x in v]))
    with open(dst, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == 'summarise':
        summarise(sys.argv[2], sys.argv[3])
    else:
        run()
