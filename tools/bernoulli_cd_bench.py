#!/usr/bin/env python
"""Timing of compute_bernoulli_grid_core_genome_cd. Prints one JSON object.

    python tools/bernoulli_cd_bench.py [--repeats 5] [--model-genes 2000]

For core-heavy tables (tools/bernoulli_bench.py's recipe) at 40,000 x 400 and 10,000 x 4,000, n_iterations = 10, both
flavours, after one warm-up call each:
  kernels_ms     per call, from the library's per-kernel events in a run of its own: the row sweeps, the column sweeps,
                 the likelihoods (bernoulli.hip's kernels, or the log flavour's own two), everything else (counts, start
                 point, table columns, statistics); and per sweep
  evaluations    of f per solve, mean and max (the two at the bounds included), and the share of solves that stop at
                 the bounds
  library_ms     the whole pgx_bernoulli_cd call (start point up, tables down, one synchronisation), median and range
  python_ms      the whole compute_bernoulli_grid_core_genome_cd call on a LightSparseDataFrame, median and range
  model          the numpy model (tests/bernoulli_cd_model.py) timed on THIS host for one iteration of the first
                 --model-genes genes of the 40,000 x 400 table (that many row solves and 400 column solves), and that time
                 scaled by solves to the full table and 10 iterations: an EXTRAPOLATION, labelled as such
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np
import scipy.sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import bernoulli_cd_model as model                         # noqa: E402
from bernoulli_bench import core_heavy                     # noqa: E402
from pangenomix_amd import _native, sparse_utils           # noqa: E402
from pangenomix_amd import pangenome_analysis as pa        # noqa: E402

LO, HI, ICP, ITERATIONS = 0.8, 0.99999999, 0.9999, 10


def spread(values):
    v = sorted(values)
    return {'median': round(v[len(v) // 2], 3), 'min': round(v[0], 3), 'max': round(v[-1], 3), 'runs': len(v)}


def split_kernels(prof, use_logs):
    def total(pred):
        return sum(ms for name, (ms, n) in prof.items() if pred(name))
    rows = total(lambda n: n.startswith('bcd_rows'))
    cols = total(lambda n: n.startswith('bcd_cols'))
    ll = total((lambda n: n in ('bcd_ll_log_kernel', 'bcd_total_kernel')) if use_logs else (lambda n: n.startswith('bern_')))
    everything = total(lambda n: n.startswith(('bcd_', 'bern_')))
    return {'row_sweeps': round(rows, 4), 'column_sweeps': round(cols, 4), 'likelihoods': round(ll, 4),
            'other': round(everything - rows - cols - ll, 4), 'per_row_sweep': round(rows / ITERATIONS, 4),
            'per_column_sweep': round(cols / ITERATIONS, 4), 'per_likelihood': round(ll / (ITERATIONS + 1), 4)}


def device_leg(ctx, repeats):
    out = {}
    for G, S in ((40000, 400), (10000, 4000)):
        rows, cols, X = core_heavy(G, S, seed=2)
        m = scipy.sparse.coo_matrix((np.ones(rows.size, dtype=np.int64), (rows, cols)), shape=(G, S))
        table = sparse_utils.LightSparseDataFrame(['g%d' % i for i in range(G)], ['s%d' % j for j in range(S)], m)
        p0 = np.clip(np.bincount(rows, minlength=G) / float(S), LO, HI)
        ctx.bernoulli_load(rows, cols, G, S)
        entry = {'present_fraction': round(float(X.mean()), 4)}
        for use_logs in (False, True):
            first = ctx.bernoulli_cd(p0, ICP, LO, HI, ITERATIONS, use_logs=use_logs)              # warm-up
            stats = ctx.bernoulli_cd_stats()
            lib_ms = []
            for _ in range(repeats):
                t0 = time.perf_counter()
                again = ctx.bernoulli_cd(p0, ICP, LO, HI, ITERATIONS, use_logs=use_logs)
                lib_ms.append((time.perf_counter() - t0) * 1e3)
                assert again.tobytes() == first.tobytes()
            ctx.profile(True)
            ctx.profile_reset()
            ctx.bernoulli_cd(p0, ICP, LO, HI, ITERATIONS, use_logs=use_logs)
            kernels = split_kernels(ctx.profile_read(), use_logs)
            ctx.profile(False)
            py_ms = []
            for _ in range(repeats):
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):
                    df = pa.compute_bernoulli_grid_core_genome_cd(table, n_iterations=ITERATIONS, use_logs=use_logs, ctx=ctx)
                py_ms.append((time.perf_counter() - t0) * 1e3)
                assert df.values.tobytes() == first.tobytes()
            on_bound = float(np.mean((first[1:, 1:] == LO) | (first[1:, 1:] == HI))) if not use_logs else None
            entry['logs' if use_logs else 'plain'] = {
                'kernels_ms': kernels, 'library_ms': spread(lib_ms), 'python_ms': spread(py_ms),
                'evaluations_per_solve_mean': round(stats['evaluations'] / float(stats['solves']), 3),
                'evaluations_per_solve_max': stats['max_evaluations'], 'solves': stats['solves'],
                'not_converged': stats['not_converged'], 'share_of_values_on_a_bound': on_bound,
                'loglikelihood_first_last': [float(first[0, 0]), float(first[0, -1])]}
        out['%dx%d' % (G, S)] = entry
    return out


def model_leg(genes):
    G, S = 40000, 400
    _, _, X = core_heavy(G, S, seed=2)
    X = X[:genes]
    p0 = np.clip(X.sum(1) / float(S), LO, HI)
    out = {}
    for use_logs in (False, True):
        t0 = time.perf_counter()
        run = model.run(X, p0, ICP, LO, HI, 1, use_logs)
        dt = time.perf_counter() - t0
        solves = genes + S
        out['logs' if use_logs else 'plain'] = {
            'measured_s': round(dt, 3), 'measured_solves': solves,
            'evaluations_per_solve_mean': round(float(run.evals.mean()), 3),
            'EXTRAPOLATED_s_40000x400_10_iterations': round(dt / solves * (G + S) * ITERATIONS, 1)}
    out['note'] = ('numpy model, all solves of a sweep side by side in arrays, one iteration of %d x %d on this host; the '
                   'full-size figure is scaled by the number of solves, not run' % (genes, S))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--model-genes', type=int, default=2000)
    a = ap.parse_args()
    ctx = _native.Context(0)
    result = {'device': ctx.device_info()['name'], 'n_iterations': ITERATIONS, 'tables': device_leg(ctx, a.repeats),
              'host_numpy_model': model_leg(a.model_genes)}
    ctx.close()
    print(json.dumps(result))


if __name__ == '__main__':
    main()
