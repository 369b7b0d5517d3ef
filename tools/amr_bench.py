#!/usr/bin/env python
"""Timing of amr.build_resistome and amr.generate_probable_hits_from_annotations with and without a device context
(DESIGN.md section 6n). Prints one JSON object.

    python tools/amr_bench.py [--runs 2] [--terms 7000] [--hits 5000] [--drugs 40] [--lines 1000000] [--out profiles/amr_bench.json]

The input is synthetic (pangenomix_amd.synth.write_amr_case): an OBO of --terms terms -- ARO:1000001, ARO:1000003, the
sixteen drug-class ids, a tree of drugs and mixtures under them, families of resistance determinants with relationships --,
an RGI table of --hits rows, --drugs drugs of interest, and an annotations file of --lines lines over --products distinct
products, one in --name-every of which names a drug, a part of a mixture or a class.
Median / min / max of --runs runs, in one process on one machine; every device result is first compared with the host's:
  resistome_device / _host            build_resistome(ctx=ctx) / (ctx=None), binary columns
  resistome_lengths_device / _host    the same with return_path_lengths=True
  probable_device / _host             generate_probable_hits_from_annotations; the host loop is timed once
  graph_reach, term_scan, dict_query  the library calls alone, on the arrays of this input (upload, kernels, download)
  kernel_ms                           per-kernel time of ONE profiled run of the three device calls (pgx_profile_read)
  nx_per_pair_extrapolated            where networkx is importable: the reference-style loop -- nx.has_path per (hit, drug) --
                                      on --nx-hits hits, multiplied up to all hits; an extrapolation, labelled as one
The host paths are THIS PROJECT'S restatement of the reference's loops (one search per distinct ARO, not per pair)."""
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

from pangenomix_amd import _native, amr, pangenome, synth           # noqa: E402


def timed(fn, runs):
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        out = fn()
        t.append(time.perf_counter() - t0)
    return {'median': float(np.median(t)), 'min': min(t), 'max': max(t)}, out


def note(what):
    print('[amr_bench] ' + what, file=sys.stderr, flush=True)


def quiet(fn, *args, **kwargs):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*args, **kwargs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=2)
    ap.add_argument('--terms', type=int, default=7000)
    ap.add_argument('--hits', type=int, default=5000)
    ap.add_argument('--drugs', type=int, default=40)
    ap.add_argument('--lines', type=int, default=1000000)
    ap.add_argument('--products', type=int, default=3000)
    ap.add_argument('--name-every', type=int, default=25)
    ap.add_argument('--nx-hits', type=int, default=100)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    ctx = _native.Context(0)
    out = {'device': ctx.device_info()['name'], 'runs': args.runs, 'terms': args.terms, 'hits': args.hits, 'drugs': args.drugs,
           'lines': args.lines, 'products': args.products, 'name_every': args.name_every,
           'host_path_is': "this project's restatement of the reference's loops (ctx=None): one search per distinct ARO"}
    with tempfile.TemporaryDirectory() as tmp:
        case = synth.write_amr_case(tmp, amr.DRUG_CLASS_AROS, n_terms=args.terms, n_hits=args.hits, n_drugs=args.drugs,
                                    n_lines=args.lines, n_products=args.products, seed=7, name_every=args.name_every)
        G, aro_names = amr.construct_aro_to_drug_network(case['obo'])
        out['graph'] = {'kind': type(G).__name__, 'nodes': len(G), 'edges': len(list(G.edges))}
        out['annotation_bytes'] = os.path.getsize(case['annotations'])
        note('inputs written: %d nodes, %d edges, %d annotation bytes' % (out['graph']['nodes'], out['graph']['edges'],
                                                                         out['annotation_bytes']))

        # build_resistome, both flavours: equal frames first, then the timings
        for lengths, label in ((False, 'resistome'), (True, 'resistome_lengths')):
            run = lambda which: quiet(amr.build_resistome, case['rgi'], case['drugs'], G, return_path_lengths=lengths,    # noqa: E731
                                      ctx=which)[1]
            amr.AMR_PATH_COUNTS.clear()
            df_d, df_h = run(ctx), run(None)
            assert dict(amr.AMR_PATH_COUNTS) == {'resistome_device': 1, 'resistome_host': 1}
            pd.testing.assert_frame_equal(df_d, df_h)
            out[label + '_device'], _ = timed(lambda: run(ctx), args.runs)
            out[label + '_host'], _ = timed(lambda: run(None), args.runs)
            out[label + '_speedup_host_median_over_device_median'] = out[label + '_host']['median'] / out[label + '_device']['median']
            note('%s: device %.3f s, host %.3f s' % (label, out[label + '_device']['median'], out[label + '_host']['median']))
        df_aro = df_h if not lengths else quiet(amr.build_resistome, case['rgi'], case['drugs'], G)[1]
        out['alleles'], out['related_cells'] = int(len(df_aro)), int(df_aro.iloc[:, 1:].notna().sum().sum())

        # generate_probable_hits_from_annotations
        kwargs = dict(G_aro=G, aro_names=aro_names, drug_to_aro=case['drug_to_aro'], manual_annots=case['manual_annots'])
        run = lambda which: quiet(amr.generate_probable_hits_from_annotations, df_aro, case['annotations'], ctx=which, **kwargs)  # noqa: E731
        amr.AMR_PATH_COUNTS.clear()
        t0 = time.perf_counter()
        prob_d = run(ctx)
        first_device = time.perf_counter() - t0
        assert dict(amr.AMR_PATH_COUNTS) == {'class_terms_device': 1, 'screen_device': 1}
        out['probable_host'], prob_h = timed(lambda: run(None), 1)
        pd.testing.assert_frame_equal(prob_d, prob_h)
        out['frames_identical'], out['probable_rows'] = True, int(len(prob_d))
        out['probable_device'], _ = timed(lambda: run(ctx), args.runs)
        out['probable_first_device_call'] = first_device
        out['probable_speedup_host_over_device_median'] = out['probable_host']['median'] / out['probable_device']['median']
        note('probable hits: device %.2f s, host %.2f s, %d rows' % (out['probable_device']['median'],
                                                                    out['probable_host']['median'], len(prob_d)))

        # the library calls alone, on the arrays of this input
        index, off, succ = amr._graph_csr(G)
        hits = pd.read_csv(case['rgi'], sep='\t')
        sources = [index['ARO:%d' % a] for a in dict.fromkeys(hits['ARO'].tolist())]
        targets = [index[a] for a in case['drugs'].values()]
        out['graph_reach'], (lengths, rounds) = timed(lambda: ctx.graph_reach(off, succ, targets, sources, return_rounds=True),
                                                      args.runs + 1)
        out['graph_reach_shape'] = {'sources': len(sources), 'targets': len(targets), 'rounds': rounds,
                                    'pairs_with_a_path': int((lengths > 0).sum()), 'longest_path_nodes': int(lengths.max())}
        data = open(case['annotations'], 'rb').read()
        arr = np.frombuffer(data, dtype=np.uint8)
        ls, le = pangenome._line_spans(arr)
        tabs = np.flatnonzero(arr == 9)
        breaks = np.sort(np.concatenate((tabs, le)))
        f_start, f_end = tabs + 1, breaks[np.searchsorted(breaks, tabs, side='right')]
        terms = sorted({t.lower().encode() for drug in case['drugs'] for t in [drug] + drug.split('/')} |
                       {n.replace('antibiotic', '').strip().encode() for n in synth.AMR_CLASS_NAMES})
        t_blob, t_off = pangenome._blob(terms)
        out['term_scan'], mask = timed(lambda: ctx.term_scan(arr, f_start.astype(np.uint64), (f_end - f_start).astype(np.uint32),
                                                             t_blob, t_off.astype(np.uint32), _native.TERM_FOLD_ASCII),
                                       args.runs + 1)
        out['term_scan_shape'] = {'fields': int(tabs.size), 'terms': len(terms), 'term_bytes': int(t_off[-1]),
                                  'fields_with_a_term': int(mask.any(axis=1).sum())}
        keys = sorted(set(data.split(b'\n')[0].split(b'\t')[1:]) | {b'hypothetical protein'})
        ctx.dict_load(*pangenome._blob(keys), want_first=False)
        fields = pangenome._spans_blob(arr, f_start, f_end)
        out['dict_query'], _ = timed(lambda: ctx.dict_query(*fields), args.runs + 1)

        # per-kernel times, a run of its own
        ctx.profile(True)
        ctx.profile_reset()
        quiet(amr.build_resistome, case['rgi'], case['drugs'], G, ctx=ctx)
        run(ctx)
        kern = {k: {'ms': ms, 'launches': n} for k, (ms, n) in ctx.profile_read().items()}
        ctx.profile(False)
        out['kernel_ms'] = kern
        out['kernel_ms_total'] = sum(v['ms'] for v in kern.values())

        try:
            import networkx as nx
        except ImportError:
            nx = None
        if nx is not None and isinstance(G, nx.DiGraph):
            some = hits['ARO'].tolist()[:args.nx_hits]
            t0 = time.perf_counter()
            found = sum(nx.has_path(G, 'ARO:%d' % a, d) for a in some for d in case['drugs'].values())
            seconds = time.perf_counter() - t0
            out['nx_per_pair_extrapolated'] = {
                'what': 'nx.has_path per (hit, drug) as the reference calls it, measured on hits_measured hits and multiplied '
                        'by hits / hits_measured: an extrapolation, not a measurement of the whole loop',
                'hits_measured': len(some), 'seconds_measured': seconds, 'pairs_with_a_path': int(found),
                'seconds_extrapolated_to_all_hits': seconds * len(hits) / max(len(some), 1)}
    ctx.close()
    text = json.dumps(out, indent=1, sort_keys=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
