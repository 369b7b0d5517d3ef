#!/usr/bin/env python
"""Timing of the gene-table / allele-table checks on the device. Prints one JSON object.

    python tools/allele_runs_bench.py [--runs 3] [--genes 150000] [--out profiles/allele_runs_bench.json]

The tables are a synthetic pair of the shape build_cds_pangenome() gives for a 400-genome set: the gene table is
synth.pancore_matrix(--genes, 400, 1); every present cell of a gene goes to one of its alleles (allele m with probability
2^-(m+1), at most 16 per gene), so the gene row is the OR of its allele rows; allele rows are ordered by their names sorted
as strings, as the pipeline orders them. Median / min / max of --runs runs after a warm-up, in one process on one machine:
  validate_gene_table, validate_gene_table_dense, extract_dominant_alleles
                       the public calls on the two LightSparseDataFrames (label parsing, run construction, upload, device
                       pass, results back, printing; extract_dominant_alleles also filters a FASTA of every allele)
  host_entry           Context.allele_runs alone with every output (the coordinates of both tables go up, all results down)
  model                tests/allele_runs_model.runs (numpy, one thread) on the dense bool tables, which it is handed ready
  kernel_ms            per-kernel time of ONE profiled host_entry call (pgx_profile_read; a run of its own)
  bytes                the allele bitmap's size and what runs_or_kernel's time makes of it as a rate, against the 8.0 TB/s
                       of HBM as a yardstick only (a 50 MB bitmap that was just written is cache-resident)
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
import scipy.sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from pangenomix_amd import _native, pangenome, sparse_utils, synth           # noqa: E402

HBM_TB_PER_S = 8.0


def timed(fn, runs, warm=True):
    if warm:
        fn()
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        out = fn()
        t.append(time.perf_counter() - t0)
    return {'median': float(np.median(t)), 'min': min(t), 'max': max(t)}, out


def quiet(fn, *args, **kwargs):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*args, **kwargs)


def synthetic_pair(n_genes, n_genomes, seed):
    """(df_genes, df_alleles) as LightSparseDataFrames."""
    rng = np.random.default_rng(seed)
    g_row, g_col, n_genes = synth.pancore_matrix(n_genes, n_genomes, seed)
    member = np.minimum(rng.geometric(0.5, g_row.size) - 1, 15)
    key, allele_of_cell = np.unique(g_row.astype(np.int64) * 16 + member, return_inverse=True)
    gene_of_allele = key // 16
    first = np.searchsorted(gene_of_allele, gene_of_allele)                  # alleles of a gene are numbered 0, 1, ...
    names = np.char.add(np.char.add(np.char.add('Syn_C', gene_of_allele.astype(str)), 'A'),
                        (np.arange(key.size) - first).astype(str))
    order = np.argsort(names, kind='stable')
    new_row = np.empty(key.size, dtype=np.int64)
    new_row[order] = np.arange(key.size)
    ones = np.ones(g_row.size, dtype=np.int64)
    genomes = np.array(['s%d' % j for j in range(n_genomes)])
    genes = sparse_utils.LightSparseDataFrame(np.char.add('Syn_C', np.arange(n_genes).astype(str)), genomes,
                                              scipy.sparse.coo_matrix((ones, (g_row, g_col)), shape=(n_genes, n_genomes)))
    alleles = sparse_utils.LightSparseDataFrame(names[order], genomes, scipy.sparse.coo_matrix(
        (ones, (new_row[allele_of_cell.ravel()], g_col)), shape=(key.size, n_genomes)))
    return genes, alleles


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--genes', type=int, default=150000)
    ap.add_argument('--genomes', type=int, default=400)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import allele_runs_model as model
    ctx = _native.Context(0)
    dfg, dfa = synthetic_pair(args.genes, args.genomes, 1)
    n_genes, n_alleles, S = dfg.shape[0], dfa.shape[0], args.genomes
    out = {'device': ctx.device_info()['name'], 'runs': args.runs, 'genes': n_genes, 'alleles': n_alleles, 'genomes': S,
           'ones': int(dfa.data.nnz)}

    with tempfile.TemporaryDirectory() as tmp:
        faa, dom = os.path.join(tmp, 'alleles.faa'), os.path.join(tmp, 'dominant.faa')
        with open(faa, 'w') as f:
            f.write(''.join('>%s\nMKTAYIAKQRQISFVKSHFS\n' % a for a in dfa.index.tolist()))
        calls = {'validate_gene_table': lambda: quiet(pangenome.validate_gene_table, dfg, dfa, ctx=ctx),
                 'validate_gene_table_dense': lambda: quiet(pangenome.validate_gene_table_dense, dfg, dfa, ctx=ctx),
                 'extract_dominant_alleles': lambda: quiet(pangenome.extract_dominant_alleles, dfa, faa, dom, ctx=ctx)}
        results = {}
        for name, fn in calls.items():
            out[name], results[name] = timed(fn, args.runs)
    assert results['validate_gene_table'] == 0 and results['validate_gene_table_dense'] == 0
    dominant = results['extract_dominant_alleles']

    # the library call alone, and the model on dense tables
    run_names, run_start = pangenome._runs_in_order(pangenome._genes_of_alleles(dfa.index))
    row_of_gene = {g: i for i, g in enumerate(dfg.index.tolist())}
    gene_of_run = np.array([row_of_gene[g] for g in run_names.tolist()], dtype=np.int32)
    a, g = dfa.data, dfg.data
    host_entry = lambda: ctx.allele_runs(a.row, a.col, n_alleles, S, run_start, g.row, g.col, n_genes, gene_of_run)   # noqa: E731
    out['host_entry'], (got, dups) = timed(host_entry, args.runs)
    assert dups == (0, 0)
    A = np.zeros((n_alleles, S), dtype=bool)
    A[a.row, a.col] = True
    G = np.zeros((n_genes, S), dtype=bool)
    G[g.row, g.col] = True
    out['model'], want = timed(lambda: model.runs(A, run_start, G, gene_of_run), max(1, min(args.runs, 2)), warm=False)
    model.assert_equal(got, want, run_names.size)
    assert dominant.index.tolist() == run_names[want['total'] > 0].tolist()
    out['runs_per_call'] = int(run_names.size)

    ctx.profile(True)
    ctx.profile_reset()
    host_entry()
    kern = {k: {'ms': ms, 'launches': n} for k, (ms, n) in ctx.profile_read().items()}
    ctx.profile(False)
    out['kernel_ms'] = kern
    out['kernel_ms_total'] = sum(v['ms'] for v in kern.values())
    bitmap = S * model.stride_words(n_alleles) * 8
    out['bytes'] = {'allele_bitmap': bitmap, 'coordinates_uploaded': int(a.nnz + g.nnz) * 8}
    ms = kern.get('runs_or_kernel', {}).get('ms', 0)
    if ms > 0:
        out['bytes']['runs_or_kernel_tb_per_s'] = bitmap / (ms * 1e-3) / 1e12
        out['bytes']['runs_or_kernel_share_of_hbm_8_tb_per_s'] = bitmap / (ms * 1e-3) / 1e12 / HBM_TB_PER_S
    out['upload_dominates_host_entry'] = out['kernel_ms_total'] * 1e-3 < 0.5 * out['host_entry']['median']
    ctx.close()
    text = json.dumps(out, indent=1, sort_keys=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
