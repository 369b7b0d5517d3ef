#!/usr/bin/env python
"""Timing of the table-against-FASTA validator and of the dictionary match under it. Prints one JSON
object.

    python tools/table_fasta_bench.py [--config cfg-3s] [--genomes N] [--runs 3] [--out profiles/table_fasta_bench.json]

The input is the synthetic protein set `--config` of pangenomix_amd.synth (cfg-3s: 400 genomes x 4,500 CDS), or its first
--genomes genomes: one FAA per genome, the exact-deduplicated sequences in genome order as the non-redundant FASTA, and the
table that records for every genome exactly its sequences, so the validator must find every genome consistent -- which is
checked first. The files are written by worker processes before the device is opened. Median / min / max of --runs runs
after a warm-up, in one process on one machine:
  kernel_ms            per-kernel time summed over ONE profiled validator run (pgx_profile_read; a run of its own)
  dict_load            Context.dict_load of all non-redundant keys: keys up, table built, first[] down
  dict_query           Context.dict_query of the first batch of genomes (TABLE_FASTA_BATCH_BYTES): queries up, last[] down
  genome_sets_diff     Context.genome_sets_diff of the whole table against itself
  host_work            the validator's host work, each piece alone on one thread: parse_nr (_fasta_records of the
                       non-redundant FASTA), parse_genomes (_genome_keys of every genome file, summed), blobs (_blob of the
                       non-redundant keys and of every batch), names (labels and headers -> bitmap rows)
  validator            validate_allele_table on all genomes; parse_share = parse_genomes / that (the parse of the next
                       genomes runs on a host thread beside the device's work, so its share of the wall time is at most this)
  restatement          tests/dict_match_model.validate, a statement-by-statement RESTATEMENT of the reference with
                       hashlib.sha256, on the first --slice genomes on the same host, run once, and its EXTRAPOLATION to all
                       genomes (the non-redundant part measured once + genomes x the per-genome part); the reference itself
                       is not available where this runs and is not timed
"""
import argparse
import contextlib
import io
import json
import multiprocessing
import os
import sys
import tempfile
import time

import numpy as np
import scipy.sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from pangenomix_amd import pangenome, sparse_utils, synth            # noqa: E402


def timed(fn, runs, warm=True):
    if warm:
        fn()
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        out = fn()
        t.append(time.perf_counter() - t0)
    return {'median': float(np.median(t)), 'min': min(t), 'max': max(t)}, out


def stage(text):
    print('table_fasta_bench: ' + text, file=sys.stderr, flush=True)


def quiet(fn, *args, **kwargs):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*args, **kwargs)


def write_genome(job):
    config, g, path = job
    ps = synth.protein_set(config)
    fams, seqs = ps.genome(g)
    with open(path, 'w') as f:
        for k, (fam, s) in enumerate(zip(fams, seqs)):
            s = s.decode('ascii')
            f.write('>%s   hypothetical protein\n' % ps.header(g, k, fam))
            f.write('\n'.join(s[i:i + 60] for i in range(0, len(s), 60)) + '\n')
    return seqs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='cfg-3s')
    ap.add_argument('--genomes', type=int, default=0)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--slice', type=int, default=8)
    ap.add_argument('--workers', type=int, default=8)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    n_genomes = args.genomes or synth.CONFIGS[args.config][0]
    out = {'config': args.config, 'genomes': n_genomes, 'runs': args.runs}

    with tempfile.TemporaryDirectory() as tmp:
        paths = [os.path.join(tmp, 'genome_%04d.faa' % g) for g in range(n_genomes)]
        t0 = time.perf_counter()
        id_of, rows, cols = {}, [], []
        with multiprocessing.Pool(args.workers) as pool:
            for g, seqs in enumerate(pool.imap(write_genome, [(args.config, g, p) for g, p in enumerate(paths)])):
                ids = {id_of.setdefault(s, len(id_of)) for s in seqs}
                rows.extend(ids)
                cols.extend([g] * len(ids))
        nr = os.path.join(tmp, 'nr.faa')
        labels = ['Syn_C%dA0' % i for i in range(len(id_of))]
        with open(nr, 'w') as f:
            for label, s in zip(labels, id_of):
                s = s.decode('ascii')
                f.write('>%s\n%s\n' % (label, '\n'.join(s[i:i + 60] for i in range(0, len(s), 60))))
        out['setup_seconds'] = time.perf_counter() - t0
        stage('%d genome files and %d non-redundant sequences written' % (n_genomes, len(labels)))
        out['records'] = n_genomes * synth.CONFIGS[args.config][1]
        out['nr_sequences'] = len(labels)
        out['table_cells'] = len(rows)
        out['genome_file_bytes'] = sum(os.path.getsize(p) for p in paths)
        names = np.array([os.path.basename(p)[:-4] for p in paths], dtype=object)
        table = sparse_utils.LightSparseDataFrame(np.array(labels, dtype=object), names, scipy.sparse.coo_matrix(
            (np.ones(len(rows), dtype=np.int64), (rows, cols)), shape=(len(labels), n_genomes)))

        from pangenomix_amd import _native                # (the device is opened after the worker processes have gone)
        ctx = _native.Context(0)
        out['device'] = ctx.device_info()['name']
        out['group_bytes'] = int(_native.lib().pgx_dict_group_bytes())
        out['batch_bytes'] = pangenome.TABLE_FASTA_BATCH_BYTES

        # the result first: every genome consistent (this is also the warm-up)
        assert quiet(pangenome.validate_allele_table, table, paths, nr, log_group=50, ctx=ctx) == 0

        stage('every genome consistent; timing the host work')
        # the host work, piece by piece
        host = {}
        host['parse_nr'], (nr_headers, nr_keys) = timed(lambda: pangenome._fasta_records(nr), args.runs, warm=False)
        t0 = time.perf_counter()
        genome_keys = [pangenome._genome_keys(p, None, {}) for p in paths]
        host['parse_genomes'] = {'seconds': time.perf_counter() - t0}
        batches, batch, size = [], [], 0
        for keys in genome_keys:
            n = sum(map(len, keys))
            if batch and size + n > pangenome.TABLE_FASTA_BATCH_BYTES:
                batches.append(batch)
                batch, size = [], 0
            batch.extend(keys)
            size += n
        batches.append(batch)
        t0 = time.perf_counter()
        nr_blob = pangenome._blob(nr_keys)
        blobs = [pangenome._blob(b) for b in batches]
        host['blobs'] = {'seconds': time.perf_counter() - t0}
        t0 = time.perf_counter()
        name_id = {}
        for r, label in enumerate(labels):
            name_id.setdefault(label, r)
        for header in nr_headers:
            name_id.setdefault(header, len(name_id))
        host['names'] = {'seconds': time.perf_counter() - t0}
        out['host_work'] = host
        out['key_bytes'] = int(nr_blob[0].size)
        out['query_bytes'] = int(sum(b[0].size for b in blobs))
        out['query_calls'] = len(blobs)
        out['first_batch'] = {'queries': len(batches[0]), 'bytes': int(blobs[0][0].size)}
        del genome_keys, batches

        stage('timing the library calls')
        # the library calls
        out['dict_load'], first = timed(lambda: ctx.dict_load(*nr_blob), args.runs)
        assert np.array_equal(first, np.arange(first.size))
        out['dict_query'], last = timed(lambda: ctx.dict_query(*blobs[0]), args.runs)
        assert (last >= 0).all()
        a_rows, a_cols = np.asarray(rows, dtype=np.int32), np.asarray(cols, dtype=np.int32)
        out['genome_sets_diff'], diff = timed(lambda: ctx.genome_sets_diff(a_rows, a_cols, a_rows, a_cols, len(labels), n_genomes),
                                              args.runs)
        assert not diff[0].any() and not diff[1].any()
        del blobs, nr_blob

        stage('timing the validator')
        # the whole validator, and one profiled run for the kernel times
        out['validator'], count = timed(lambda: quiet(pangenome.validate_allele_table, table, paths, nr, log_group=50, ctx=ctx),
                                        args.runs, warm=False)
        assert count == 0
        out['validator']['per_genome'] = out['validator']['median'] / n_genomes
        out['validator']['parse_share'] = host['parse_genomes']['seconds'] / out['validator']['median']
        ctx.profile(True)
        ctx.profile_reset()
        quiet(pangenome.validate_allele_table, table, paths, nr, log_group=50, ctx=ctx)
        kern = {k: {'ms': ms, 'launches': n} for k, (ms, n) in ctx.profile_read().items()}
        ctx.profile(False)
        out['kernel_ms'] = kern
        out['kernel_ms_total'] = sum(v['ms'] for v in kern.values())
        out['validator']['kernel_share'] = out['kernel_ms_total'] * 1e-3 / out['validator']['median']
        ctx.close()

        stage('timing the restatement')
        # the SHA-256 restatement on a slice
        import dict_match_model as model
        n_slice = min(args.slice, n_genomes)
        cells = {(r, c): 1 for r, c in zip(rows, cols) if c < n_slice}
        t0 = time.perf_counter()
        model.validate(labels, list(names), cells, [], nr)
        t_nr = time.perf_counter() - t0
        t0 = time.perf_counter()
        text = model.validate(labels, list(names), cells, paths[:n_slice], nr)
        t_slice = time.perf_counter() - t0
        assert text.endswith('Feature Table Inconsistencies: 0\n')
        per_genome = (t_slice - t_nr) / n_slice
        out['restatement'] = {'what': "statement-by-statement restatement of the reference with hashlib.sha256 "
                                      "(tests/dict_match_model.validate), not the reference itself",
                              'slice_genomes': n_slice, 'seconds_nr_part': t_nr, 'seconds_slice': t_slice,
                              'seconds_per_genome': per_genome,
                              'seconds_extrapolated_to_all_genomes': t_nr + per_genome * n_genomes}
    text = json.dumps(out, indent=1, sort_keys=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
