#!/usr/bin/env python
"""Timing of weboflife.get_node_gene_content_table with and without a device context, and of pgx_tree_content alone
(DESIGN.md section 6p). Prints one JSON object.

    python tools/weboflife_bench.py [--species 10000] [--genes 20000] [--runs 3] [--out profiles/weboflife_bench.json]

The input is synthetic (pangenomix_amd.synth.phylogeny): a random tree with polytomies over --species species, a twentieth
as many mapped inner nodes and unmapped leaves, and a gene x species table of --genes genes. The device frame is first
compared with the host's, value for value (nan with nan), and WEBOFLIFE_PATH_COUNTS must name the device path. Then, in one
process, after one warm-up call each, medians of --runs calls:
  tree_content        ONE library call with its transfers, on the first chunk of genes (as many as fit 256 MiB of counts),
                      into a fresh array per call and into one kept buffer, which is how the table function calls it
  kernels             the sum of that call's kernels from the library's own profile slots (a run of its own), the number of
                      launches (= the tree's heights), the time per launch, and the rate the sum makes of
                      2 x n_nodes x stride x 4 bytes (every row written once and read once), against the 8.0 TB/s of HBM
  table_device/_host  the whole get_node_gene_content_table with ctx and with ctx=None (--host-runs calls)
  table_stages        where the time of ONE device call goes: the traversal, reading the table, numbering the nodes, the
                      library calls, and the rest (the division and the frame), host clocks around each
  single_gene         the restated get_node_gene_content on --single genes, and that time x genes / --single: an
                      EXTRAPOLATION, which stands in for the reference (the same loop, one gene per call)"""
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

from pangenomix_amd import _native, synth                          # noqa: E402
from pangenomix_amd import weboflife as wol                        # noqa: E402

HBM_TB_PER_S = 8.0


def timed(fn, runs):
    t, out = [], None
    for _ in range(runs):
        out = None                                                   # (the last result goes before the next one comes)
        t0 = time.perf_counter()
        out = fn()
        t.append(time.perf_counter() - t0)
    return {'median': float(np.median(t)), 'min': min(t), 'max': max(t), 'runs': runs}, out


def note(what):
    print('[weboflife_bench] ' + what, file=sys.stderr, flush=True)


class Clocked(object):
    """a context whose library calls are timed and whose first call's arguments are kept"""

    def __init__(self, ctx):
        self.ctx, self.seconds, self.calls, self.first = ctx, 0.0, 0, None

    def tree_content_workspace_bytes(self, *a):
        return self.ctx.tree_content_workspace_bytes(*a)

    def tree_content(self, *a, **kw):
        if self.first is None:
            self.first = a
        t0 = time.perf_counter()
        out = self.ctx.tree_content(*a, **kw)
        self.seconds += time.perf_counter() - t0
        self.calls += 1
        return out


def same_frames(a, b, block=1024):
    assert list(a.index) == list(b.index) and list(a.columns) == list(b.columns)
    x, y = a.to_numpy(), b.to_numpy()
    return all(np.array_equal(x[:, lo:lo + block], y[:, lo:lo + block], equal_nan=True) for lo in range(0, x.shape[1], block))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--species', type=int, default=10000)
    ap.add_argument('--genes', type=int, default=20000)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--host-runs', type=int, default=1)
    ap.add_argument('--single', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    ctx = _native.Context(0)
    t0 = time.perf_counter()
    G, root, m, tab = synth.phylogeny(args.species, 1, n_genes=args.genes, max_children=4, mapped_internal=args.species // 20,
                                      unmapped_leaves=args.species // 20)
    out = {'device': ctx.device_info()['name'], 'species': args.species, 'genes': args.genes, 'nodes': len(G),
           'ones_in_table': int(tab.data.nnz), 'input_made_s': time.perf_counter() - t0,
           'host_path_is': "this project's ctx=None path: numpy rows over genes, a Python loop over nodes"}
    note('%d nodes, %d ones' % (len(G), tab.data.nnz))

    # the device path once, clocked, then the comparison with the host's frame
    wol.WEBOFLIFE_PATH_COUNTS.clear()
    clocked = Clocked(ctx)
    t0 = time.perf_counter()
    got = wol.get_node_gene_content_table(G, tab, m, root, ctx=clocked)
    out['table_first_device_call'] = time.perf_counter() - t0
    assert dict(wol.WEBOFLIFE_PATH_COUNTS) == {'table_device': 1}, dict(wol.WEBOFLIFE_PATH_COUNTS)
    out['chunks'], out['genes_per_chunk'] = clocked.calls, wol._chunk_genes(len(G))
    out['table_host'], want = timed(lambda: wol.get_node_gene_content_table(G, tab, m, root), args.host_runs)
    assert same_frames(got, want)
    out['nan_rows'] = int(np.isnan(want.iloc[:, 0].to_numpy()).sum())
    del got, want
    note('device frame equals host frame; host %.2f s' % out['table_host']['median'])
    out['table_device'], _ = timed(lambda: wol.get_node_gene_content_table(G, tab, m, root, ctx=ctx), args.runs)
    del _

    # where one device call's time goes
    stages = {}
    t0 = time.perf_counter()
    nodes = wol.__get_bfs_traversal__(G, root)[::-1]
    stages['traversal'] = time.perf_counter() - t0
    t0 = time.perf_counter()
    table = wol._GeneTable(tab, None)
    stages['reading_the_table'] = time.perf_counter() - t0
    t0 = time.perf_counter()
    plan = wol._device_plan(G, nodes, m, table)
    stages['numbering_and_heights'] = time.perf_counter() - t0
    clocked = Clocked(ctx)
    t0 = time.perf_counter()
    frame = wol.get_node_gene_content_table(G, tab, m, root, ctx=clocked)
    stages['whole_call'] = time.perf_counter() - t0
    stages['library_calls'] = clocked.seconds
    stages['division_records_and_frame'] = stages['whole_call'] - clocked.seconds - stages['traversal'] - stages['reading_the_table'] \
        - stages['numbering_and_heights']
    stages['host_share'] = 1.0 - clocked.seconds / stages['whole_call']
    out['table_stages'] = stages
    out['levels'] = int(plan[4].size - 1)
    out['edges'] = int(plan[2].size)
    del frame
    out['speedup_host_median_over_device_median'] = out['table_host']['median'] / out['table_device']['median']
    note('device %.2f s (library %.2f s), host %.2f s' % (out['table_device']['median'], clocked.seconds, out['table_host']['median']))

    # the library call alone, on the first chunk
    a = clocked.first
    n_genes = a[2]
    stride = ctx.tree_content_stride(n_genes)
    ctx.tree_content(*a, return_totals=True)
    out['tree_content'], _ = timed(lambda: ctx.tree_content(*a, return_totals=True), args.runs + 2)
    del _
    out['tree_content'].update(genes=int(n_genes), records=int(a[0].size), counts_bytes=int(4 * stride * len(nodes)))
    kept = np.empty((len(nodes), stride), dtype=np.uint32)           # as the table function calls it: one buffer, pages faulted in once
    ctx.tree_content(*a, return_totals=True, counts=kept)
    out['tree_content_into_a_kept_buffer'], _ = timed(lambda: ctx.tree_content(*a, return_totals=True, counts=kept), args.runs + 2)
    del _, kept
    ctx.profile(True)
    ctx.profile_reset()
    ctx.tree_content(*a, return_totals=True)
    kern = {k: {'ms': ms, 'launches': n} for k, (ms, n) in ctx.profile_read().items()}
    ctx.profile(False)
    tree_ms = sum(v['ms'] for k, v in kern.items() if k.startswith('tree_'))
    launches = sum(v['launches'] for k, v in kern.items() if k.startswith('tree_'))
    traffic = 2 * len(nodes) * stride * 4
    out['kernels'] = {'per_kernel': kern, 'tree_kernels_ms': tree_ms, 'launches': launches, 'ms_per_launch': tree_ms / max(launches, 1),
                      'traffic_bytes': traffic, 'tb_per_s': traffic / (tree_ms * 1e-3) / 1e12 if tree_ms else None,
                      'share_of_hbm_8_tb_per_s': traffic / (tree_ms * 1e-3) / 1e12 / HBM_TB_PER_S if tree_ms else None}

    # the single-gene function, extrapolated
    dense = pd.DataFrame(tab.islice(i_indices=np.arange(args.single)).values, index=tab.index[:args.single], columns=tab.columns)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        t0 = time.perf_counter()
        for gene in dense.index:
            wol.get_node_gene_content(G, dense.loc[gene], m, root)
        took = time.perf_counter() - t0
    out['single_gene'] = {'genes': args.single, 'seconds': took, 'EXTRAPOLATED_to_all_genes_s': took * args.genes / args.single,
                          'note': 'the restated get_node_gene_content, one gene per call; the figure for all genes is an extrapolation'}
    ctx.close()
    text = json.dumps(out, indent=1, sort_keys=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
