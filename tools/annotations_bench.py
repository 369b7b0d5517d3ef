#!/usr/bin/env python
"""Timing of extract_annotations and generate_annotations with and without a device context. Prints
one JSON object.

    python tools/annotations_bench.py [--runs 2] [--genomes 400] [--features 4500] [--out profiles/annotations_bench.json]

The input is --genomes synthetic GFF files of --features CDS lines each (the line format of tools/proximal_bench.py) whose
products are drawn from --products strings, one in four percent-encoded, and the allele-names file a pipeline would have
written for them: one gene per feature; a tenth of the genes have one allele that lists every genome (a row of --genomes
ids), three tenths two to four alleles, the rest an allele per genome (a run of --genomes rows of one id). One record in
twenty carries another product than its gene's, so alleles differ and votes are not unanimous.
Median / min / max of --runs runs, in one process on one machine:
  device_path   extract_annotations(ctx=ctx), batch 100: everything, from reading the GFFs to the written file
  host_path     extract_annotations() -- THIS PROJECT'S restatement of the reference's loop, the code without ctx; the
                reference itself cannot run on Python 3 (urllib.unquote), so it is not timed
  parse_gffs    _parse_gff_regular + _annotation_keys over all GFFs: the host work the device path starts with
  dict_load_keys, dict_query_fids, annot_vote   the library calls alone, on the arrays of this input (upload, kernels, download)
  kernel_ms     per-kernel time of ONE profiled extract_annotations(ctx=ctx) (pgx_profile_read; a run of its own)
  generate_*    generate_annotations for --generate-features feature names on the file written above
Before anything is timed both paths run once and the files they wrote are compared byte for byte."""
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

from pangenomix_amd import _native, pangenome           # noqa: E402


def timed(fn, runs):
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        out = fn()
        t.append(time.perf_counter() - t0)
    return {'median': float(np.median(t)), 'min': min(t), 'max': max(t)}, out


def note(what):
    print('[annotations_bench] ' + what, file=sys.stderr, flush=True)


def quiet(fn, *args, **kwargs):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*args, **kwargs)


def write_inputs(tmp, args):
    """(gff paths, allele names path)"""
    rng = np.random.default_rng(1)
    words = ['protein', 'kinase', 'transporter', 'subunit', 'family', 'putative', 'ABC', 'ribosomal', 'tRNA', 'synthase',
             'permease', 'regulator', 'binding', 'membrane', 'oxidase', 'reductase', 'phage', 'domain', '(EC 2.7.7.6)', "5'-end,"]
    pool = []
    for i in range(args.products):
        text = ' '.join(words[int(j)] for j in rng.integers(0, len(words), int(rng.integers(2, 6)))) + ' %d' % i
        if i % 4 == 0:
            text = text.replace(' ', '%20').replace('(', '%28').replace(')', '%29').replace(',', '%2C').replace("'", '%27')
        pool.append(text)
    base = rng.integers(0, len(pool), args.features)
    gffs = []
    for g in range(args.genomes):
        product = np.where(rng.integers(0, 20, args.features) == 0, rng.integers(0, len(pool), args.features), base)
        path = os.path.join(tmp, 'g%d.gff' % g)
        with open(path, 'w') as f:
            f.write('##gff-version 3\n' + ''.join(
                'accn|contig%d\tPATRIC\tCDS\t%d\t%d\t.\t+\t0\tID=fig|g%d.peg.%d;locus_tag=G%d_%05d;product=%s\n'
                % (k % 50, 1 + 1000 * k, 900 + 1000 * k, g, k, g, k, pool[int(product[k])]) for k in range(args.features)))
        gffs.append(path)
    names = os.path.join(tmp, 'Syn_allele_names.tsv')
    rows = 0
    with open(names, 'w') as f:
        for k in range(args.features):
            fid = ['fig|g%d.peg.%d|G%d_%05d' % (g, k, g, k) for g in range(args.genomes)]
            kind = k % 10
            if kind == 0:
                groups = [fid]
            elif kind <= 3:
                n = int(rng.integers(2, 5))
                groups = [fid[i::n] for i in range(n)]
            else:
                groups = [[x] for x in fid]
            for a, members in enumerate(groups):
                f.write('Syn_C%dA%d\t%s\n' % (k, a, '\t'.join(members)))
            rows += len(groups)
    return gffs, names, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=2)
    ap.add_argument('--genomes', type=int, default=400)
    ap.add_argument('--features', type=int, default=4500)
    ap.add_argument('--products', type=int, default=3000)
    ap.add_argument('--generate-features', type=int, default=100000)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    ctx = _native.Context(0)
    out = {'device': ctx.device_info()['name'], 'runs': args.runs, 'genomes': args.genomes, 'features': args.features,
           'products': args.products, 'gff_lines': args.genomes * args.features, 'batch': 100,
           'host_path_is': "this project's restatement of the reference's loop (ctx=None); the reference cannot run on Python 3"}
    with tempfile.TemporaryDirectory() as tmp:
        gffs, names, rows = write_inputs(tmp, args)
        out['allele_rows'] = rows
        note('inputs written: %d GFF lines, %d allele rows' % (out['gff_lines'], rows))
        out_h, out_d = os.path.join(tmp, 'host.tsv'), os.path.join(tmp, 'device.tsv')

        # both paths once: identical files, or nothing is timed (these runs are the warm-up, and the host path's only one
        # when --runs is 1)
        pangenome.ANNOTATION_PATH_COUNTS.clear()
        t0 = time.perf_counter()
        quiet(pangenome.extract_annotations, gffs, names, out_d, ctx=ctx)
        first_device = time.perf_counter() - t0
        assert dict(pangenome.ANNOTATION_PATH_COUNTS) == {'extract_device': 1}
        t0 = time.perf_counter()
        quiet(pangenome.extract_annotations, gffs, names, out_h)
        first_host = time.perf_counter() - t0
        assert open(out_h, 'rb').read() == open(out_d, 'rb').read(), 'the two paths wrote different files'
        out['files_identical'], out['output_bytes'] = True, os.path.getsize(out_h)
        out['first_call'] = {'device_path': first_device, 'host_path': first_host}
        note('identical files; first calls: device %.2f s, host %.2f s' % (first_device, first_host))

        out['device_path'], _ = timed(lambda: quiet(pangenome.extract_annotations, gffs, names, out_d, ctx=ctx), args.runs)
        note('device path: %.2f s' % out['device_path']['median'])
        out['host_path'], _ = timed(lambda: quiet(pangenome.extract_annotations, gffs, names, out_h), max(args.runs - 1, 1))
        note('host path: %.2f s' % out['host_path']['median'])
        out['speedup_host_median_over_device_median'] = out['host_path']['median'] / out['device_path']['median']

        # the pieces
        def parse_all():
            return [pangenome._annotation_keys(pangenome._parse_gff_regular(open(p, 'rb').read()), False, None) for p in gffs]
        out['parse_gffs'], parts = timed(parse_all, args.runs)
        out['parse_names'], parsed = timed(lambda: pangenome._parse_names_regular(open(names, 'rb').read()), args.runs)
        keys, key_off = pangenome._join_blobs([(p[0], p[1]) for p in parts])
        fids, fid_off = pangenome._spans_blob(parsed['arr'], *parsed['fid'])
        out['n_keys'], out['n_fids'] = int(key_off.size - 1), int(fid_off.size - 1)
        out['dict_load_keys'], _ = timed(lambda: ctx.dict_load(keys, key_off), args.runs + 1)
        out['dict_query_fids'], last = timed(lambda: ctx.dict_query(fids, fid_off), args.runs + 1)
        assert (last >= 0).all()
        # the vote alone, on ids that stand for the raw products (the decoded ones differ by nothing that matters to it)
        products, product_off = pangenome._join_blobs([(p[3], p[4]) for p in parts])
        tok = ctx.dict_load(products, product_off)[last]
        row_off = np.zeros(parsed['n'] + 1, dtype=np.uint64)
        np.cumsum(parsed['n_fids'], out=row_off[1:])
        a_start = parsed['allele'][0]
        genes = pangenome._fixed_width(parsed['arr'], a_start, parsed['gene_end'] - a_start)
        run_off = np.concatenate((np.flatnonzero(np.concatenate(([True], genes[1:] != genes[:-1]))), [parsed['n']])).astype(np.uint32)
        out['annot_vote'], voted = timed(lambda: ctx.annot_vote(tok, row_off, run_off), args.runs + 1)
        out['n_rows'], out['n_runs'], out['rows_that_differ'] = int(parsed['n']), int(run_off.size - 1), int(voted[3].sum())

        # generate_annotations on the file just written
        rng = np.random.default_rng(2)
        features = ['Syn_C%d%s' % (int(k), '' if v == 0 else 'AUD'[v - 1] + str(int(n))) for k, v, n in zip(
            rng.integers(0, args.features + 50, args.generate_features), rng.integers(0, 4, args.generate_features),
            rng.integers(0, args.genomes, args.generate_features))]
        got = []
        for which, label in ((ctx, 'generate_device'), (None, 'generate_host')):
            out[label], series = timed(lambda: pangenome.generate_annotations(features, [out_h], ctx=which), args.runs)
            got.append(series)
        assert got[0].equals(got[1])
        out['generate_features'], out['generate_found'] = len(features), int(got[0].notna().sum())

        # per-kernel times, a run of its own
        ctx.profile(True)
        ctx.profile_reset()
        quiet(pangenome.extract_annotations, gffs, names, out_d, ctx=ctx)
        kern = {k: {'ms': ms, 'launches': n} for k, (ms, n) in ctx.profile_read().items()}
        ctx.profile(False)
        out['kernel_ms'] = kern
        out['kernel_ms_total'] = sum(v['ms'] for v in kern.values())
    ctx.close()
    text = json.dumps(out, indent=1, sort_keys=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
