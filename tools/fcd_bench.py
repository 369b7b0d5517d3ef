#!/usr/bin/env python
"""Timing of formal_concept_decomposition on the device. Prints one JSON object.

    python tools/fcd_bench.py [--runs 5] [--out profiles/fcd_bench.json]

For synth.pancore_matrix(150000, 400, 1), decomposed completely and with limit=100, and for the 12,000 x 100 table of
the fixture:
  call_s             wall time of the public call (W, H and F; median, min, max of --runs runs after a warm-up)
  concepts_s         the same for the concepts alone (fcd._concepts: upload, device loop, F as tuples; no dense W / H)
  concepts, steps    concepts found and score evaluations (one masked popcount of every live column each)
  steps_per_s        steps / median concepts_s
  algorithmic_tb_per_s   steps x n_genomes x stride_words x 8 bytes / median concepts_s -- the bitmap is CACHE-RESIDENT
                     (L2 / Infinity Cache), so this is set against the 8.0 TB/s of HBM only as a yardstick, as
                     BASELINE.md does for pan/core
  kernel_ms, score_kernel_share   per-kernel time of ONE profiled run (pgx_profile_read; its own run: the events slow
                     the host loop) and the share of fcd_score_kernel in the kernels' total
Beside it, in the same run: model_12000x100_s, tests/fcd_model.py (numpy, one thread) on the 12,000 x 100 table -- the
CPU figure the device call on that table is set against.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from pangenomix_amd import _native, fcd, synth           # noqa: E402

HBM_TB_PER_S = 8.0


def table(n_rows, n_cols):
    r, c, G = synth.pancore_matrix(n_rows, n_cols, 1)
    return scipy.sparse.coo_matrix((np.ones(r.size, dtype=np.int64), (r, c)), shape=(G, n_cols))


def timed(fn, runs):
    fn()                                                   # warm-up
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        out = fn()
        t.append(time.perf_counter() - t0)
    return {'median': float(np.median(t)), 'min': min(t), 'max': max(t)}, out


def measure(ctx, coo, limit, runs):
    n_rows, n_cols = coo.shape
    stride = _native.lib().pgx_bitmap_stride_words(n_rows)
    call, (W, H, F) = timed(lambda: fcd.formal_concept_decomposition(coo, limit=limit, ctx=ctx), runs)
    del W, H
    concepts, (F2, _, info) = timed(lambda: fcd._concepts(coo, limit=limit, ctx=ctx), runs)
    steps = info['steps']
    ctx.profile(True)
    ctx.profile_reset()
    fcd._concepts(coo, limit=limit, ctx=ctx)
    kern = {k: ms for k, (ms, n) in ctx.profile_read().items() if k.startswith('fcd_') or k == 'presence_bitmap_kernel'}
    ctx.profile(False)
    total = sum(kern.values())
    return {'shape': [n_rows, n_cols], 'limit': limit, 'call_s': call, 'concepts_s': concepts, 'concepts': len(F),
            'steps': steps, 'ones': info['ones_total'], 'ones_left': info['ones_left'],
            'steps_per_s': steps / concepts['median'],
            'algorithmic_tb_per_s_cache_resident': steps * n_cols * stride * 8 / concepts['median'] / 1e12,
            'share_of_hbm_8_tb_per_s': steps * n_cols * stride * 8 / concepts['median'] / 1e12 / HBM_TB_PER_S,
            'kernel_ms': kern, 'score_kernel_share': kern.get('fcd_score_kernel', 0.0) / total if total else 0.0,
            'kernels_share_of_concepts_s': total * 1e-3 / concepts['median']}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import fcd_model
    ctx = _native.Context(0)
    out = {'device': ctx.device_info()['name'], 'runs': args.runs}
    small = table(12000, 100)
    out['12000x100_limit400'] = measure(ctx, small, 400, args.runs)
    dense = small.toarray()
    t0 = time.perf_counter()
    F_model, steps_model = fcd_model.decompose(dense, limit=400, return_steps=True)
    out['model_12000x100_s'] = time.perf_counter() - t0
    out['model_12000x100'] = {'concepts': len(F_model), 'steps': steps_model}
    assert fcd._concepts(small, limit=400, ctx=ctx)[0] == F_model
    out['device_faster_than_model_12000x100'] = out['12000x100_limit400']['call_s']['median'] < out['model_12000x100_s']
    big = table(150000, 400)
    out['150000x400_limit100'] = measure(ctx, big, 100, args.runs)
    out['150000x400_full'] = measure(ctx, big, None, args.runs)
    ctx.close()
    text = json.dumps(out, indent=1, sort_keys=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
