#!/usr/bin/env python
"""Timing of the direct UTR table validator and of the window scan under it. Prints one JSON object.

    python tools/window_scan_bench.py [--runs 3] [--genomes 400] [--out profiles/window_scan_bench.json]

The input is one synthetic genome: --bases (5 Mbp) of random ACGT in --contigs (50) contigs of unequal length, and --sequences
(4,500) table sequences of window 53 cut from it, every second one from the reverse strand. The 400-genome run gives the
validator that genome under 400 file names (links to one file, so the disk holds 5 MB, not 2 GB; every file is opened, read
and parsed again) and a table in which every genome has every sequence. Median / min / max of --runs runs after a warm-up,
in one process on one machine:
  kernel_ms            per-kernel time of ONE profiled window_scan call (pgx_profile_read; a run of its own)
  window_scan          Context.window_scan alone: text and keys go up, the scan, found comes down
  genome_host_work     what the validator does around that call for one genome: parse_fna (load_sequences_from_fasta),
                       check_and_join (the 256-entry check of every contig, the join), keys (_scan_keys)
  validator            validate_upstream_table_direct on --genomes genomes, once; parse_share = genomes x parse_fna / that
                       (the parse of genome g + 1 runs on a host thread beside the scan of genome g, so its share of the
                       wall time is at most this)
  restatement          tests/window_scan_model.validate_direct, a plain-Python RESTATEMENT of the reference's loop (one
                       iteration per base and strand, str slices, a dict), on ONE genome on the same host, run once; the
                       reference itself is not available where this runs
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

from pangenomix_amd import _native, pangenome, sparse_utils           # noqa: E402

WINDOW = 53


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


def synthetic_genome(n_bases, n_contigs, n_sequences, seed):
    rng = np.random.default_rng(seed)
    nt = np.frombuffer(b'ACGT', dtype=np.uint8)
    cuts = np.sort(rng.choice(np.arange(1000, n_bases - 1000), n_contigs - 1, replace=False))
    bases = nt[rng.integers(0, 4, n_bases)].tobytes().decode()
    contigs = [bases[a:b] for a, b in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [n_bases]]))]
    seqs = {}
    while len(seqs) < n_sequences:
        c = contigs[int(rng.integers(0, n_contigs))]
        if len(c) < WINDOW:
            continue
        s = int(rng.integers(0, len(c) - WINDOW + 1))
        seq = c[s:s + WINDOW]
        seqs[pangenome.reverse_complement(seq) if len(seqs) % 2 else seq] = None
    return contigs, list(seqs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--genomes', type=int, default=400)
    ap.add_argument('--bases', type=int, default=5000000)
    ap.add_argument('--contigs', type=int, default=50)
    ap.add_argument('--sequences', type=int, default=4500)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import window_scan_model as model
    ctx = _native.Context(0)
    contigs, seqs = synthetic_genome(args.bases, args.contigs, args.sequences, 1)
    labels = ['Syn_C%dU0' % i for i in range(len(seqs))]
    out = {'device': ctx.device_info()['name'], 'runs': args.runs, 'genomes': args.genomes, 'bases': args.bases,
           'contigs': args.contigs, 'sequences': len(seqs), 'window': WINDOW}

    with tempfile.TemporaryDirectory() as tmp:
        first = os.path.join(tmp, 'g0.fna')
        with open(first, 'w') as f:
            for i, c in enumerate(contigs):
                f.write('>contig%d\n' % i + '\n'.join(c[j:j + 80] for j in range(0, len(c), 80)) + '\n')
        paths = [first]
        for g in range(1, args.genomes):
            paths.append(os.path.join(tmp, 'g%d.fna' % g))
            os.symlink(first, paths[-1])
        nr = os.path.join(tmp, 'nr.fna')
        with open(nr, 'w') as f:
            f.write(''.join('>%s\n%s\n' % (a, s) for a, s in zip(labels, seqs)))

        # one genome, piece by piece
        host = {}
        host['parse_fna'], parsed = timed(lambda: pangenome.load_sequences_from_fasta(first), args.runs)
        parsed = list(parsed.values())
        host['check_and_join'], text = timed(lambda: b'\x00'.join(pangenome._check_contig(c) for c in parsed), args.runs)
        host['keys'], (keys, fwd, rev) = timed(lambda: pangenome._scan_keys(seqs, WINDOW), args.runs)
        out['genome_host_work'] = host
        out['text_bytes'], out['keys'] = len(text), int(keys.shape[0])
        out['window_scan'], found = timed(lambda: ctx.window_scan(text, keys), max(args.runs, 5))
        hit = np.concatenate([found.astype(bool), [False]])
        assert (hit[fwd] | hit[rev]).all()            # every sequence occurs on one strand; half the keys do not occur
        ctx.profile(True)
        ctx.profile_reset()
        ctx.window_scan(text, keys)
        kern = {k: {'ms': ms, 'launches': n} for k, (ms, n) in ctx.profile_read().items()}
        ctx.profile(False)
        out['kernel_ms'] = kern
        out['kernel_ms_total'] = sum(v['ms'] for v in kern.values())
        ms = kern.get('scan_kernel', {}).get('ms', 0)
        if ms > 0:
            out['scan_kernel_gb_per_s'] = len(text) / (ms * 1e-3) / 1e9
            out['scan_kernel_bytes_hashed_per_s'] = len(text) * WINDOW / (ms * 1e-3)

        # the validator on all genomes, once, and the restatement on one
        n = len(seqs)
        rows = np.repeat(np.arange(n), args.genomes)
        cols = np.tile(np.arange(args.genomes), n)
        names = np.array([os.path.basename(p)[:-4] for p in paths], dtype=object)
        table = sparse_utils.LightSparseDataFrame(np.array(labels, dtype=object), names, scipy.sparse.coo_matrix(
            (np.ones(rows.size, dtype=np.int64), (rows, cols)), shape=(n, args.genomes)))
        quiet(pangenome.validate_upstream_table_direct, table, paths[:2], nr, ctx=ctx)             # warm-up
        t0 = time.perf_counter()
        missing = quiet(pangenome.validate_upstream_table_direct, table, paths, nr, log_group=50, ctx=ctx)
        wall = time.perf_counter() - t0
        assert missing == 0
        out['validator'] = {'seconds': wall, 'per_genome': wall / args.genomes,
                            'parse_share': args.genomes * host['parse_fna']['median'] / wall,
                            'window_scan_share': args.genomes * out['window_scan']['median'] / wall}
        t0 = time.perf_counter()
        text_out = model.validate_direct(labels, ['g0'], [(i, 0) for i in range(n)], [first], nr, (-50, 3), 'upstream')
        out['restatement'] = {'seconds_one_genome': time.perf_counter() - t0, 'what': 'plain-Python restatement of the '
                              "reference's loop (tests/window_scan_model.validate_direct), not the reference itself"}
        assert '\tMissing' not in text_out
        out['restatement']['seconds_extrapolated_to_all_genomes'] = out['restatement']['seconds_one_genome'] * args.genomes
    ctx.close()
    text = json.dumps(out, indent=1, sort_keys=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
