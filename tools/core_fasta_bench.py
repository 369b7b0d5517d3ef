#!/usr/bin/env python
"""Timing of create_core_genes_fasta on the device. Prints one JSON object; there is no pass/fail time.

    python tools/core_fasta_bench.py [--runs 3] [--genes 150000] [--out profiles/core_fasta_bench.json]

The tables are the synthetic 400-genome pair of tools/allele_runs_bench.py, written to disk the way build_cds_pangenome
writes them (.npz + label files) together with a FASTA file of every allele; the thresholds are the eight of the
reference's README (400, 396, 392, 388, 384, 380, 200, 60). Median / min / max of --runs runs after a warm-up, in one
process on one machine:
  one_call             create_core_genes_fasta with the eight thresholds and eight output files: ONE pass over the tables,
                       one library call, one pass over the FASTA file
  eight_calls          the same files from eight scalar calls (what the README tells the user to do)
  one_call_split / eight_calls_split
                       where one run of each spends its time: reading the tables and labels, grouping the rows, the library
                       call (Context.core_select), names, the FASTA pass; `kernel_ms` is the per-kernel time inside the
                       one library call and `eight_calls_kernel_ms_total` all kernels of the eight (pgx_profile_read,
                       runs of their own)
  numpy_chain          a pandas/numpy restatement of the reference's chain (groupby sizes, isin, one sort by gene and
                       maximum.reduceat, a set for the FASTA filter) for ONE threshold on the same host; times eight for
                       the README's loop, since every repetition re-reads everything
  reference_chain      the reference's OWN algorithm (iterrows with two .loc[list] per gene; `name in list` per FASTA
                       record), restated here line for line, on the first --ref-genes genes only: it is quadratic, so it is
                       timed on a subset that finishes and EXTRAPOLATED -- linearly in the genes for the iterrows loops,
                       by records x names for the FASTA filter. An extrapolation, reported as such.
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
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from allele_runs_bench import synthetic_pair, timed           # noqa: E402
from pangenomix_amd import _native, core_genome               # noqa: E402

README_THRESHOLDS = (400, 396, 392, 388, 384, 380, 200, 60)


def quiet(fn, *args, **kwargs):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*args, **kwargs)


def write_inputs(tmp, dfg, dfa):
    files = {}
    for tag, df in (('allele', dfa), ('gene', dfg)):
        path = os.path.join(tmp, 'Syn_strain_by_%s.npz' % tag)
        m = df.data.tocoo()
        np.savez(path, row=m.row.astype(np.int32), col=m.col.astype(np.int32), format=np.bytes_('coo'),
                 shape=np.asarray(m.shape, dtype=np.int64), data=np.ones(m.nnz, dtype=np.int64))
        with open(path + '.labels.txt', 'w') as f:
            f.write('\n'.join(df.index.tolist() + df.columns.tolist()) + '\n')
        files[tag + '_npz'], files[tag + '_labels'] = path, path + '.labels.txt'
    files['faa'] = os.path.join(tmp, 'Syn_nr.faa')
    with open(files['faa'], 'w') as f:
        seq = 'MKTAYIAKQRQISFVKSHFSRQLEERLGLIEVQAPILSRVGDGTQDNLSGAEKAVQVKVK'      # 60 residues: one line either way
        f.write(''.join('>%s\n%s\n' % (a, seq) for a in dfa.index.tolist()))
    return files


def split_run(files, nums, outs, ctx):
    """One run of the workflow, step by step with the module's own pieces: seconds per step."""
    t = [time.perf_counter()]
    tables = core_genome._core_tables(files['allele_npz'], files['allele_labels'], files['gene_npz'], files['gene_labels'])
    t.append(time.perf_counter())
    a_rows, a_cols, a_shape, allele_labels, gene_labels, g_rows, g_cols = tables
    run_start, gene_of_run, new_row, old_row = core_genome._allele_groups(gene_labels, allele_labels)
    t.append(time.perf_counter())
    out, dups = ctx.core_select(new_row[a_rows], a_cols, a_shape[0], a_shape[1], run_start, core_genome._thresholds(nums),
                                gene_rows=g_rows, gene_genomes=g_cols, n_genes=gene_labels.size, gene_of_run=gene_of_run,
                                want=('gene_count', 'selected', 'n_selected'))
    t.append(time.perf_counter())
    names = [allele_labels[old_row[sel]] for sel in out['selected']]
    t.append(time.perf_counter())
    core_genome._filter_fasta(files['faa'], names, outs)
    t.append(time.perf_counter())
    steps = ('read_tables_and_labels', 'group_rows', 'library_call', 'names', 'fasta_pass')
    return dict(zip(steps, np.diff(t).tolist())), [int(n) for n in out['n_selected']]


def numpy_chain(files, genomes_num, out_faa):
    """The reference's chain for one threshold, vectorised (no device)."""
    with np.load(files['allele_npz']) as z:
        a_rows = z['row']
    with np.load(files['gene_npz']) as z:
        g_rows = z['row']
    allele_count = np.bincount(a_rows)
    gene_count = np.bincount(g_rows)
    gene_df = pd.read_csv(files['gene_labels'], header=None, names=['gene_name'])
    allele_df = pd.read_csv(files['allele_labels'], header=None, names=['allele_name'])
    gene_df['gene'] = gene_df.index
    allele_df['gene_name'] = allele_df['allele_name'].str.extract(r'([^A]+)')
    merged = pd.merge(allele_df, gene_df, on='gene_name', how='left')
    gene = merged['gene'].values
    rows = np.flatnonzero(~np.isnan(gene) & (gene < gene_count.size))
    rows = rows[rows < allele_count.size]
    core = np.flatnonzero(gene_count >= genomes_num)
    rows = rows[np.isin(gene[rows].astype(np.int64), core)]
    rows = rows[np.argsort(gene[rows], kind='stable')]
    g = gene[rows].astype(np.int64)
    starts = np.flatnonzero(np.concatenate([[True], g[1:] != g[:-1]]))
    counts = allele_count[rows]
    top = np.maximum.reduceat(counts, starts)
    lengths = np.diff(np.concatenate([starts, [rows.size]]))
    is_top = np.flatnonzero(counts == np.repeat(top, lengths))
    run_of = np.repeat(np.arange(starts.size), lengths)[is_top]
    best = rows[is_top[np.concatenate([[True], run_of[1:] != run_of[:-1]])]]
    names = set(allele_df['allele_name'].values[best].tolist())
    with open(files['faa']) as f, open(out_faa, 'w') as out:
        keep = False
        for line in f:
            if line[0] == '>':
                keep = line[1:].split(None, 1)[0].split('|')[0] in names
            if keep:
                out.write(line)
    return len(names)


def reference_chain(files, genomes_num, n_ref_genes, allele_labels, gene_labels):
    """The reference's own loops on the first n_ref_genes genes: seconds of the iterrows part and of the FASTA filter, and
    the sizes the extrapolation needs."""
    with np.load(files['allele_npz']) as z:
        a_rows = z['row']
    with np.load(files['gene_npz']) as z:
        g_rows = z['row']
    gene_names = pd.Series(allele_labels).str.extract(r'([^A]+)')[0]
    gene_of = pd.Series(np.arange(gene_labels.size), index=gene_labels).reindex(gene_names.values).values
    keep = np.flatnonzero(gene_of < n_ref_genes)
    pairs = pd.DataFrame({'gene': gene_of[keep].astype(np.int64), 'allele': keep}).groupby('gene')['allele'].agg(list).reset_index()
    pairs.columns = ['gene', 'allele_index']
    row_counts_df = pd.DataFrame({'allele_index': np.arange(np.bincount(a_rows).size), 'count': np.bincount(a_rows)})
    gene_occurrence = pd.DataFrame({'gene_index': np.arange(np.bincount(g_rows).size), 'count': np.bincount(g_rows)})
    gene_occurrence = gene_occurrence[gene_occurrence['gene_index'] < n_ref_genes]
    t0 = time.perf_counter()
    core = []
    for _, row in gene_occurrence.iterrows():                                # find_core_genes
        if row['count'] >= genomes_num:
            core.append({'gene_index': row['gene_index'], 'highest_expression': row['count']})
    core = pd.DataFrame(core)
    subset = pairs[pairs['gene'].isin(core['gene_index'].unique())].copy() if len(core) else pairs.iloc[:0]
    best = []
    for _, row in subset.iterrows():                                         # find_highest_allele_expression
        idx = row['allele_index']
        highest = row_counts_df.loc[idx, 'count'].idxmax()
        row_counts_df.loc[idx, 'count'].duplicated().any()
        best.append({'gene': row['gene'], 'highest_expression': highest})
    t1 = time.perf_counter()
    names = [allele_labels[b['highest_expression']] for b in best]
    n_records = 0
    with open(files['faa']) as f:                                            # filter_sequences: `name in list` per record
        for line in f:
            if line[0] == '>':
                n_records += 1
                if n_records > 20000:
                    break
                line[1:].split(None, 1)[0].split('|')[0] in names
    t2 = time.perf_counter()
    return {'genes': int(n_ref_genes), 'iterrows_s': t1 - t0, 'names': len(names), 'fasta_records_timed': min(n_records, 20000),
            'fasta_filter_s': t2 - t1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--genes', type=int, default=150000)
    ap.add_argument('--genomes', type=int, default=400)
    ap.add_argument('--ref-genes', type=int, default=3000)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    ctx = _native.Context(0)
    dfg, dfa = synthetic_pair(args.genes, args.genomes, 1)
    nums = [x for x in README_THRESHOLDS if x <= args.genomes] or [args.genomes]
    out = {'device': ctx.device_info()['name'], 'runs': args.runs, 'genes': int(dfg.shape[0]), 'alleles': int(dfa.shape[0]),
           'genomes': args.genomes, 'thresholds': nums}
    with tempfile.TemporaryDirectory() as tmp:
        files = write_inputs(tmp, dfg, dfa)
        outs = [os.path.join(tmp, 'core_%d.faa' % k) for k in nums]
        args5 = (files['allele_npz'], files['allele_labels'], files['gene_npz'], files['gene_labels'], files['faa'])
        out['one_call'], _ = timed(lambda: quiet(core_genome.create_core_genes_fasta, *args5, nums, outs, ctx=ctx), args.runs)
        together = [open(p, 'rb').read() for p in outs]

        def eight():
            for k, p in zip(nums, outs):
                quiet(core_genome.create_core_genes_fasta, *args5, k, p, ctx=ctx)
        out['eight_calls'], _ = timed(eight, args.runs)
        assert together == [open(p, 'rb').read() for p in outs], 'one call and eight calls wrote different files'
        out['one_call_split'], out['selected_per_threshold'] = split_run(files, nums, outs, ctx)
        parts = [split_run(files, [k], [p], ctx)[0] for k, p in zip(nums, outs)]
        out['eight_calls_split'] = {k: float(sum(p[k] for p in parts)) for k in parts[0]}
        ctx.profile(True)
        ctx.profile_reset()
        split_run(files, nums, outs, ctx)
        out['kernel_ms'] = {k: {'ms': ms, 'launches': n} for k, (ms, n) in ctx.profile_read().items()}
        out['kernel_ms_total'] = sum(v['ms'] for v in out['kernel_ms'].values())
        ctx.profile_reset()
        for k, p in zip(nums, outs):
            split_run(files, [k], [p], ctx)
        out['eight_calls_kernel_ms_total'] = sum(ms for ms, _ in ctx.profile_read().values())
        ctx.profile(False)

        check = os.path.join(tmp, 'numpy.faa')
        k = nums[len(nums) // 2]
        out['numpy_chain'], n_names = timed(lambda: numpy_chain(files, k, check), args.runs)
        out['numpy_chain']['threshold'] = k
        out['numpy_chain']['times_eight'] = 8 * out['numpy_chain']['median']
        assert n_names == out['selected_per_threshold'][nums.index(k)]
        assert open(check, 'rb').read() == together[nums.index(k)], 'the numpy chain wrote another file'

        ref = reference_chain(files, nums[-1], min(args.ref_genes, dfg.shape[0]), np.asarray(dfa.index), np.asarray(dfg.index))
        scale = dfg.shape[0] / float(ref['genes'])
        names_full = out['selected_per_threshold'][-1]
        per_test = ref['fasta_filter_s'] / max(ref['fasta_records_timed'] * max(ref['names'], 1), 1)
        ref['extrapolated'] = {'threshold': nums[-1], 'iterrows_s': ref['iterrows_s'] * scale,
                               'fasta_filter_s': per_test * dfa.shape[0] * names_full * 0.5,
                               'how': 'iterrows: linear in the genes; filter: seconds per (record x name) on the subset times '
                                      'records x names / 2 (a hit stops half way through the list on average; a miss walks all of it)'}
        ref['extrapolated']['total_s'] = ref['extrapolated']['iterrows_s'] + ref['extrapolated']['fasta_filter_s']
        out['reference_chain'] = ref
    ctx.close()
    text = json.dumps(out, indent=1, sort_keys=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
