#!/usr/bin/env python
"""Timing of compute_bernoulli_grid_core_genome's device evaluation and of the whole call (DESIGN.md section on the
Bernoulli likelihood). Prints one JSON object.

    python tools/bernoulli_bench.py [--evals 50] [--skip-cpu]

  device     per-evaluation kernel time (sum of the library's kernels, from its per-kernel events), cells/s, for
             core-heavy tables at 40,000 x 400 and 10,000 x 4,000 in the default mode and with every present cell's own
             log (PGX_BERNOULLI_EXACT), and for an all-absent / all-present table (the cost of an absent and a present
             cell)
  whole      the whole call at both shapes, split into device kernels, the rest of the evaluation calls (copies of P, Q
             and the result, launch and sync) and everything else (scipy's L-BFGS-B and the Python around it)
  cpu        one evaluation of the model's likelihood and gradient with dense G x S numpy temporaries (the
             reference's way of evaluating them) at 40,000 x 400, on this host
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

from pangenomix_amd import _native, sparse_utils           # noqa: E402
from pangenomix_amd import pangenome_analysis as pa        # noqa: E402


def core_heavy(G, S, seed=0):
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.6, 1.0, G)
    q = rng.uniform(0.97, 1.0, S)
    X = rng.random((G, S)) < np.outer(p, q)
    rows, cols = np.nonzero(X)
    return rows.astype(np.int32), cols.astype(np.int32), X


def kernel_ms(ctx):
    return sum(ms for name, (ms, n) in ctx.profile_read().items() if name.startswith('bern_'))


def time_evals(ctx, G, S, n, exact):
    rng = np.random.default_rng(1)
    pq = np.concatenate((rng.uniform(0.8, 0.999, G), rng.uniform(0.95, 0.9999, S)))
    ctx.bernoulli_eval(pq, exact=exact)                     # warm-up
    ctx.profile(True)
    ctx.profile_reset()
    t0 = time.perf_counter()
    for _ in range(n):
        ctx.bernoulli_eval(pq, exact=exact)
    wall = (time.perf_counter() - t0) / n * 1e3
    dev = kernel_ms(ctx) / n
    ctx.profile(False)
    return {'kernel_ms': round(dev, 4), 'eval_wall_ms': round(wall, 4), 'cells_per_s': G * S / (dev * 1e-3)}


def device_leg(ctx, n):
    out = {}
    for G, S in ((40000, 400), (10000, 4000)):
        rows, cols, X = core_heavy(G, S)
        ctx.bernoulli_load(rows, cols, G, S)
        key = '%dx%d' % (G, S)
        out[key] = {'present_fraction': round(float(X.mean()), 4), 'fast': time_evals(ctx, G, S, n, False),
                    'exact': time_evals(ctx, G, S, n, True)}
    G, S = 40000, 400
    ctx.bernoulli_load(np.zeros(0, np.int32), np.zeros(0, np.int32), G, S)
    out['all_absent_40000x400'] = time_evals(ctx, G, S, n, False)
    r, c = np.divmod(np.arange(G * S, dtype=np.int64), S)
    ctx.bernoulli_load(r.astype(np.int32), c.astype(np.int32), G, S)
    out['all_present_40000x400'] = {'fast': time_evals(ctx, G, S, n, False), 'exact': time_evals(ctx, G, S, n, True)}
    return out


def whole_leg(ctx):
    out = {}
    for G, S in ((40000, 400), (10000, 4000)):
        rows, cols, _ = core_heavy(G, S, seed=2)
        m = scipy.sparse.coo_matrix((np.ones(rows.size, dtype=np.int64), (rows, cols)), shape=(G, S))
        table = sparse_utils.LightSparseDataFrame(['g%d' % i for i in range(G)], ['s%d' % j for j in range(S)], m)
        spent = [0.0, 0]
        real = _native.Context.bernoulli_eval

        def timed(self, pq, exact=False):
            t = time.perf_counter()
            try:
                return real(self, pq, exact)
            finally:
                spent[0] += time.perf_counter() - t
                spent[1] += 1
        _native.Context.bernoulli_eval = timed
        ctx.profile(True)
        ctx.profile_reset()
        try:
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                df_opt, res = pa.compute_bernoulli_grid_core_genome(table, ctx=ctx)
            total = time.perf_counter() - t0
        finally:
            _native.Context.bernoulli_eval = real
        dev = kernel_ms(ctx) * 1e-3
        ctx.profile(False)
        out['%dx%d' % (G, S)] = {'total_s': round(total, 4), 'device_kernels_s': round(dev, 4),
                                 'eval_calls_other_s': round(spent[0] - dev, 4),
                                 'host_rest_s': round(total - spent[0], 4), 'evaluations': spent[1],
                                 'nit': int(res.nit), 'nfev': int(res.nfev), 'status': int(res.status)}
    return out


def cpu_leg():
    G, S = 40000, 400
    _, _, X = core_heavy(G, S, seed=2)
    X = X.astype(np.int64)
    rng = np.random.default_rng(1)
    P, Q = rng.uniform(0.8, 0.999, G), rng.uniform(0.95, 0.9999, S)
    t0 = time.perf_counter()
    r = P[:, None] * Q[None, :]
    absent = 1.0 - X
    ll = (X * np.log(r)).sum() + (absent * np.log(1.0 - r)).sum()
    t1 = time.perf_counter()
    w = absent / (1.0 - P[:, None] * Q[None, :])
    gp = X.sum(1) / P - (w * Q[None, :]).sum(1)
    gq = X.sum(0) / Q - (w * P[:, None]).sum(0)
    t2 = time.perf_counter()
    assert np.isfinite(ll) and np.isfinite(gp).all() and np.isfinite(gq).all()
    return {'40000x400': {'loglikelihood_s': round(t1 - t0, 4), 'gradient_s': round(t2 - t1, 4),
                          'threads': os.environ.get('OMP_NUM_THREADS')}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--evals', type=int, default=50)
    ap.add_argument('--skip-cpu', action='store_true')
    a = ap.parse_args()
    ctx = _native.Context(0)
    result = {'device': ctx.device_info()['name'], 'evaluation': device_leg(ctx, a.evals), 'whole_call': whole_leg(ctx)}
    if not a.skip_cpu:
        result['cpu_numpy_evaluation'] = cpu_leg()
    ctx.close()
    print(json.dumps(result))


if __name__ == '__main__':
    main()
