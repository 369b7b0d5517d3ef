#!/usr/bin/env python
"""Timing of compute_concept_list_similarity on the device against the host loop ("Comparing two
decompositions"). Prints one JSON object.

    python tools/fcd_similarity_bench.py [--runs 5] [--host-budget-s 600] [--out profiles/fcd_similarity_bench.json]

Two cases, both decompositions made on the device first (not timed):
  12000x100_limit400   synth.pancore_matrix(12000, 100, 1), limit=400: F against F with seed=1
  150000x400_full      synth.pancore_matrix(150000, 400, 1), complete: plain against seed=1
For each:
  python_call_s   compute_concept_list_similarity(F1, F2, S, ctx=ctx): lists in, score out (median, min, max of --runs
                  runs after a warm-up)
  library_call_s  Context.fcd_match on the flattened lists: upload, kernels, results back
  kernel_ms       per kernel, from the library's own events (pgx_profile_read) in runs of their own: median, min, max of
                  the total over one call, and the launches of one call
  overlap_word_pairs_per_s   concepts paired x len(F2) x (row + column mask words) / median fcd_overlap_kernel time. The
                  masks are cache-resident at these sizes, so the figure is set against the VALU (5 lane-operations per
                  word pair in the compiled inner loop, 64 per CU and clock), not against HBM.
  host_loop_s     the host loop (ctx=None) timed here, in the same run on the same machine. When a timing of the first 20
                  concepts of F1 predicts more than --host-budget-s seconds for all of them, only that prefix is timed
                  and host_loop_s is EXTRAPOLATED from it ('host_loop': 'extrapolated from the first 20 concepts'),
                  in proportion to the pairs the loop visits.
The device's score is asserted equal to the host loop's (on the same lists: all of F1, or its first 20 concepts) before any
time is reported, and the run fails unless the device path's Python call is faster than the host loop.
"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np
import scipy.sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pangenomix_amd import _native, fcd, synth           # noqa: E402

PREFIX = 20
VALU_OPS_PER_WORD_PAIR = 5        # the inner loop as compiled: 128 v_and_b32 + 128 v_bcnt_u32_b32 + 64 v_add3_u32 per 64 word pairs


def table(n_rows, n_cols):
    r, c, G = synth.pancore_matrix(n_rows, n_cols, 1)
    return scipy.sparse.coo_matrix((np.ones(r.size, dtype=np.int64), (r, c)), shape=(G, n_cols))


def spread(t):
    return {'median': float(np.median(t)), 'min': float(min(t)), 'max': float(max(t))}


def timed(fn, runs):
    fn()                                                   # warm-up
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        out = fn()
        t.append(time.perf_counter() - t0)
    return spread(t), out


def measure(ctx, coo, limit, runs, host_budget_s):
    n_rows, n_cols = coo.shape
    F1 = fcd.formal_concept_decomposition(coo, limit=limit, ctx=ctx)[2]
    F2 = fcd.formal_concept_decomposition(coo, limit=limit, seed=1, ctx=ctx)[2]
    n1, n2, k = len(F1), len(F2), min(len(F1), len(F2))
    out = {'shape': [n_rows, n_cols], 'limit': limit, 'concepts': [n1, n2],
           'mean_rows_per_concept': float(np.mean([len(x) for x, _ in F1]))}

    # the host loop first: the whole of it, or its first concepts when the whole would take too long
    t0 = time.perf_counter()
    host_prefix = fcd.compute_concept_list_similarity(F1[:PREFIX], F2, coo)
    t_prefix = time.perf_counter() - t0
    pairs = lambda n: sum(n2 - i for i in range(min(n, n2)))           # noqa: E731  (pairs the loop visits)
    predicted = t_prefix * pairs(n1) / max(pairs(PREFIX), 1)
    assert fcd.compute_concept_list_similarity(F1[:PREFIX], F2, coo, ctx=ctx) == host_prefix
    out['host_loop_first_%d_s' % PREFIX] = t_prefix
    if predicted <= host_budget_s:
        print('host loop on %d x %d concepts: about %.0f s' % (n1, n2, predicted), file=sys.stderr)
        done = threading.Event()

        def progress():                                    # a line every 30 s: the loop itself says nothing for minutes
            t = time.perf_counter()
            while not done.wait(30.0):
                print('host loop: %.0f s' % (time.perf_counter() - t), file=sys.stderr)

        ticker = threading.Thread(target=progress, daemon=True)
        ticker.start()
        t0 = time.perf_counter()
        host_score = fcd.compute_concept_list_similarity(F1, F2, coo)
        out['host_loop_s'] = time.perf_counter() - t0
        done.set()
        ticker.join()
        out['host_loop'] = 'measured'
        assert fcd.compute_concept_list_similarity(F1, F2, coo, ctx=ctx) == host_score
    else:
        out['host_loop_s'] = predicted
        out['host_loop'] = 'extrapolated from the first %d concepts' % PREFIX
    out['score'] = fcd.compute_concept_list_similarity(F1, F2, coo, ctx=ctx)

    out['python_call_s'], _ = timed(lambda: fcd.compute_concept_list_similarity(F1, F2, coo, ctx=ctx), runs)
    lists = fcd._flatten(F1) + fcd._flatten(F2)
    lists = tuple(a.astype(np.int32) if i % 2 == 0 else a for i, a in enumerate(lists))
    out['library_call_s'], res = timed(lambda: ctx.fcd_match(n_rows, n_cols, *lists), runs)
    assert res[2] / float(np.sum(coo)) == out['score']

    ctx.profile(True)
    per_run = []
    for _ in range(runs + 1):
        ctx.profile_reset()
        ctx.fcd_match(n_rows, n_cols, *lists)
        per_run.append({name: v for name, v in ctx.profile_read().items() if name.startswith('fcd_')})
    ctx.profile(False)
    per_run = per_run[1:]                                               # (the first is the warm-up)
    out['kernel_ms'] = {name: dict(spread([r[name][0] for r in per_run]), launches=per_run[0][name][1])
                        for name in sorted(per_run[0])}
    lib = _native.lib()
    words = int(lib.pgx_bitmap_stride_words(n_rows)) + int(lib.pgx_bitmap_stride_words(n_cols))
    rate = k * n2 * words / (out['kernel_ms']['fcd_overlap_kernel']['median'] * 1e-3)
    info = ctx.device_info()
    valu = info['compute_units'] * 64 * info['clock_khz'] * 1e3 / VALU_OPS_PER_WORD_PAIR    # 64 lane-operations per CU and clock
    out['overlap_word_pairs_per_s'] = rate
    out['overlap_share_of_valu_ceiling'] = rate / valu
    out['overlap_tiles'] = [-(-n2 // 32) * -(-min(k - b, 256) // 32) for b in range(0, k, 256)]
    out['workspace_bytes'] = ctx.fcd_match_workspace_bytes(n_rows, n_cols, n1, n2)
    out['speedup_python_call'] = out['host_loop_s'] / out['python_call_s']['median']
    out['device_faster_than_host_loop'] = out['python_call_s']['median'] < out['host_loop_s']
    assert out['device_faster_than_host_loop']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--host-budget-s', type=float, default=600.0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    ctx = _native.Context(0)
    info = ctx.device_info()
    out = {'device': info['name'], 'compute_units': info['compute_units'], 'clock_khz': info['clock_khz'],
           'runs': args.runs, 'host_budget_s': args.host_budget_s}
    out['12000x100_limit400'] = measure(ctx, table(12000, 100), 400, args.runs, args.host_budget_s)
    out['150000x400_full'] = measure(ctx, table(150000, 400), None, args.runs, args.host_budget_s)
    ctx.close()
    text = json.dumps(out, indent=1, sort_keys=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
