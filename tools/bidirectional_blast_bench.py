#!/usr/bin/env python
"""Timing of ncbi.bidirectional_blast and of the Smith-Waterman kernels under it. Prints one JSON object.

    python tools/bidirectional_blast_bench.py [--runs 3] [--proteins 4500] [--out profiles/bidirectional_blast_bench.json]

The input is synthetic (pangenomix_amd.synth, the source of the tests' fixtures): genome 0 of the protein set `cfg-2s` cut to
--proteins proteins, and synth.related_protein_set of it (a tenth substituted, one planted indel in half of the proteins,
unrelated flanks, 15 % absent). Recorded, in one process on one machine:
  candidate_pairs, cells         of the 5-mer join; cells = sum of len(q) * len(s) over the pairs
  score_pass, stats_pass         kernel time of ONE profiled library call (pgx_profile_read) and GCUPS = cells / time; the pass
                                 with statistics over the pairs that reached min_score, whose share and cells are recorded
  sw_pairs                       the library call with its transfers and the host's ordering of the pairs: median / min / max
                                 of --runs runs after a warm-up
  call                           bidirectional_blast on the two files with a Context, split into reading, join, library call
                                 (with the thresholds and the path split around it) and report writing
  host_sw                        the model timed on --host-sample pairs (score-only pass, then statistics where reported) and
                                 EXTRAPOLATED by cells to all pairs: an estimate, not a measurement
"""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pangenomix_amd import _native, ncbi, synth           # noqa: E402
from pangenomix_amd.cluster import read_fasta_for_clustering   # noqa: E402


def note(*words):
    print(*words, file=sys.stderr, flush=True)


def spread(t):
    return {'median': float(np.median(t)), 'min': float(min(t)), 'max': float(max(t))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--proteins', type=int, default=4500)
    ap.add_argument('--host-sample', type=int, default=40)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    base = synth.protein_set('cfg-2s').genome(0)[1][:args.proteins]
    names2, set2, _ = synth.related_protein_set(base, seed=1)
    work = tempfile.mkdtemp(prefix='blast_bench_')
    a = synth.write_protein_fasta(os.path.join(work, 'a.faa'), ['a%d' % i for i in range(len(base))], base)
    b = synth.write_protein_fasta(os.path.join(work, 'b.faa'), names2, set2)
    ids1, res1, off1, _ = read_fasta_for_clustering(a)
    ids2, res2, off2, _ = read_fasta_for_clustering(b)
    len1, len2 = np.diff(off1.astype(np.int64)), np.diff(off2.astype(np.int64))
    result = {'proteins': [len(ids1), len(ids2)], 'residues': [int(len1.sum()), int(len2.sum())], 'runs': args.runs}

    t = []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        pa, pb = ncbi.candidate_pairs(res1, off1, res2, off2, 5)
        t.append(time.perf_counter() - t0)
    cells = len1[pa] * len2[pb]
    result.update(candidate_pairs=int(pa.size), cells=int(cells.sum()), join_host_s=spread(t))
    note('pairs', pa.size, 'cells', int(cells.sum()), 'join', result['join_host_s'])
    min_score = ncbi.min_scores(len1[pa], len2[pb], int(len1.sum()), int(len2.sum()), ncbi.DEFAULT_EVALUE)

    ctx = _native.Context(0)
    rows = ctx.sw_pairs(res1, off1, res2, off2, pa, pb, min_score)                 # warm-up: the workspace grows here
    n_stats = ctx.sw_last_stats_pairs()
    with_stats = (rows[:, 0] > 0) & (rows[:, 0] >= min_score)
    assert int(with_stats.sum()) == n_stats
    t = []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        ctx.sw_pairs(res1, off1, res2, off2, pa, pb, min_score)
        t.append(time.perf_counter() - t0)
    result['sw_pairs_s'] = spread(t)
    ctx.profile(True)
    ctx.profile_reset()
    ctx.sw_pairs(res1, off1, res2, off2, pa, pb, min_score)
    kernels = {k: v[0] for k, v in ctx.profile_read().items() if k.startswith('sw_')}
    ctx.profile(False)
    stats_cells = int(cells[with_stats].sum())
    result['kernel_ms'] = kernels
    result['score_pass'] = {'ms': kernels['sw_score_kernel'], 'cells': int(cells.sum()),
                            'gcups': float(cells.sum()) / kernels['sw_score_kernel'] / 1e6}
    result['stats_pass'] = {'ms': kernels['sw_stats_kernel'], 'pairs': n_stats, 'share_of_pairs': n_stats / max(int(pa.size), 1),
                            'cells': stats_cells, 'gcups': stats_cells / kernels['sw_stats_kernel'] / 1e6}
    note('kernels', kernels, 'sw_pairs', result['sw_pairs_s'], 'stats pairs', n_stats)

    calls = []
    for _ in range(args.runs):
        timings = {}
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            ncbi.bidirectional_blast(a, b, os.path.join(work, 'device'), ctx=ctx, timings=timings)
        timings['total_s'] = time.perf_counter() - t0
        calls.append(timings)
    result['call'] = {k: spread([c[k] for c in calls]) for k in ('total_s', 'read_s', 'join_s', 'align_s', 'write_s')}
    result['call']['report_lines'] = [sum(1 for _ in open(os.path.join(work, 'device', n)))
                                      for n in ('a_to_b.tsv', 'b_to_a.tsv')]
    note('call', result['call'])

    # the model on a sample spread over the pairs by cells, extrapolated by cells
    rng = np.random.default_rng(0)
    sample = rng.choice(pa.size, size=min(args.host_sample, pa.size), replace=False)
    sample = np.concatenate([sample, np.flatnonzero(with_stats)[:args.host_sample // 4]])
    t0 = time.perf_counter()
    host = ncbi.align_pairs(res1, off1, res2, off2, pa[sample], pb[sample], min_score[sample], ctx=None)
    host_s = time.perf_counter() - t0
    assert np.array_equal(host, rows[sample]), 'host model and device disagree on the sample'
    per_cell = host_s / float((cells[sample] * np.where(with_stats[sample], 2, 1)).sum())
    result['host_sw'] = {'sample_pairs': int(sample.size), 'sample_s': host_s,
                         'extrapolated_s_all_pairs': per_cell * float(cells.sum() + stats_cells),
                         'note': 'EXTRAPOLATION by cells from the sample; the sample equals the device rows'}
    note('host_sw', result['host_sw'])
    text = json.dumps(result, indent=1, sort_keys=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps(result, sort_keys=True))


if __name__ == '__main__':
    main()
