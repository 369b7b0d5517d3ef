#!/usr/bin/env python
"""Timing of the Monte-Carlo KS test of compute_beta_binomial_core_genome. Prints one JSON object.

    python tools/betabinom_bench.py [--iters 1000,10000,100000] [--numpy-iters 1000]

For a 400-genome counts Series (about 3,400 genes in the 100 fitted points) and a 4,000-genome one (about 10,500 genes in
250 points), at each iteration count:
  kernel_us_per_iter   bbn_ks_kernel time per iteration (the library's per-kernel events)
  ks_call_s            the whole ks_montecarlo_bbn call (host generation, copies, kernels)
  h2d_bytes            bytes of generator words the call uploads (8 per draw)
  estimator_s          the whole compute_beta_binomial_core_genome call with ks_iter = that count
Once per case:
  host_words_per_s     the host generator alone (pgx_legacy_uniform_words into a reused buffer)
  h2d_gb_per_s         a page-locked host-to-device copy of 256 MiB (torch, device events)
  numpy_loop_s         this repository's numpy restatement of the reference's loop (np.random.choice, then a
                       histogram, cumsum and max per iteration) at --numpy-iters iterations, on this host
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pangenomix_amd import _native                         # noqa: E402
from pangenomix_amd import pangenome_analysis as pa        # noqa: E402


def counts_series(seed, n_genomes, n_core, n_acc, a, b):
    rng = np.random.default_rng(seed)
    core = n_genomes - rng.binomial(n_genomes, rng.beta(a, b, n_core))
    counts = np.concatenate((rng.integers(1, n_genomes, n_acc), core))
    vals, tally = np.unique(counts, return_counts=True)
    return pd.Series(tally.astype(np.int64), index=vals.astype(np.int64))


CASES = {'400_genomes': (counts_series(1, 400, 3400, 600, 0.5, 60.0), 100),
         '4000_genomes': (counts_series(2, 4000, 11000, 1000, 0.8, 40.0), 250)}


def numpy_loop(model_cdf, probs, n_samples, iterations):
    L = probs.size
    draws = np.random.choice(np.arange(L), size=n_samples * iterations, p=probs).reshape(iterations, n_samples)
    out = np.empty(iterations)
    for i in range(iterations):
        hist = np.bincount(draws[i], minlength=L).astype(np.float64)
        out[i] = np.max(np.abs(np.cumsum(hist) / hist.sum() - model_cdf))
    return out


def host_rate(n_words=1 << 26):
    key = np.random.get_state()[1].copy()
    _native.legacy_uniform_words(key, 624, 1 << 20)
    t0 = time.perf_counter()
    _native.legacy_uniform_words(key, 624, n_words)
    return n_words / (time.perf_counter() - t0)


def h2d_rate(nbytes=1 << 28):
    import torch
    src = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
    dst = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    dst.copy_(src, non_blocking=True)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(4):
        dst.copy_(src, non_blocking=True)
    e1.record()
    torch.cuda.synchronize()
    return 4 * nbytes / (e0.elapsed_time(e1) * 1e-3) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', default='1000,10000,100000')
    ap.add_argument('--numpy-iters', type=int, default=1000)
    args = ap.parse_args()
    warnings.simplefilter('ignore')
    ctx = _native.Context(0)
    out = {'device': ctx.device_info()['name'], 'host_words_per_s': host_rate(), 'h2d_gb_per_s': h2d_rate()}
    for name, (counts, n_points) in CASES.items():
        n_genomes = max(counts.index)
        misses, fields, sim_limit = pa._beta_binomial_fit(counts, n_genomes, n_points, 0.999)
        a, b = fields['alpha'], fields['beta']
        n_samples = int(misses.sum())
        case = {'n_samples': n_samples, 'sim_limit': int(sim_limit), 'alpha': a, 'beta': b}
        np.random.seed(0)
        pa.ks_montecarlo_bbn(misses, n_genomes, a, b, iterations=10, sim_limit=sim_limit, ctx=ctx)     # warm-up
        for iters in (int(x) for x in args.iters.split(',')):
            ctx.profile(True)
            ctx.profile_reset()
            t0 = time.perf_counter()
            pa.ks_montecarlo_bbn(misses, n_genomes, a, b, iterations=iters, sim_limit=sim_limit, ctx=ctx)
            ks_s = time.perf_counter() - t0
            kern_ms = sum(ms for k, (ms, n) in ctx.profile_read().items() if k.startswith('bbn_'))
            ctx.profile(False)
            t0 = time.perf_counter()
            pa.compute_beta_binomial_core_genome(None, df_counts=counts, num_points=n_points, ks_iter=iters, ctx=ctx)
            est_s = time.perf_counter() - t0
            case[str(iters)] = {'kernel_us_per_iter': kern_ms * 1e3 / iters, 'kernel_ms': kern_ms, 'ks_call_s': ks_s,
                                'h2d_bytes': 8 * n_samples * iters, 'estimator_s': est_s}
        model_cdf = np.cumsum(np.exp(pa.betabin_logpmf(np.arange(sim_limit), n_genomes, a, b)))
        probs = pa._bbn_probs(n_genomes, a, b, sim_limit)
        t0 = time.perf_counter()
        numpy_loop(model_cdf, probs, n_samples, args.numpy_iters)
        case['numpy_loop_s'] = {str(args.numpy_iters): time.perf_counter() - t0}
        out[name] = case
    ctx.close()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
