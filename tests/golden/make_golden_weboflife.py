"""Writes tests/golden/weboflife: what the reference's get_node_gene_content and draw_nx_dendrogram (weboflife.py:16-143)
returned on a hand-written tree of 41 nodes, a map of its nodes to 12 species and a table of 9 genes. Needs the reference
checkout -- its directory is the first argument or $PANGENOMIX_REFERENCE; nothing of it is copied -- and networkx and
matplotlib, which the reference imports. Only data is written: edges.tsv and edges_small.tsv (parent, child, length, in
insertion order), mrca_to_species.tsv, genes_pa.tsv and expected.json.

The tree holds: a polytomy at the root and one of four leaves; a mapped internal node (M0) with a subtree below it; unmapped
leaves (U0, U1), one of them the only child of its parent (U2 below N13, so that N13 is nan too); species mapped by two or
three nodes; a species (S11) that no node maps; children inserted out of name order. The table holds a gene in no species,
one in every species and seven drawn ones.
Recorded: the reference's dict per gene as ordered pairs with nan as null; for each irregular input of
tests/weboflife_cases.py the exception's type, or the dict where the reference returns one; for two trees the depths (the
values the reference passes through round(), caught by giving its module a `round` of its own), node_xy, and how many lines
and arcs it drew."""
import importlib.util
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else os.environ['PANGENOMIX_REFERENCE']
sys.path.insert(0, os.path.dirname(HERE))
os.environ.setdefault('MPLBACKEND', 'Agg')

import matplotlib                                         # noqa: E402
matplotlib.use('Agg')
import networkx as nx                                     # noqa: E402
import pandas as pd                                       # noqa: E402

_spec = importlib.util.spec_from_file_location('ref_weboflife', os.path.join(REFERENCE, 'pangenomix', 'weboflife.py'))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)

import weboflife_cases as cases                           # noqa: E402

OUT = cases.GOLDEN
TREE = [('N0', ['N2', 'N1', 'N3']), ('N1', ['N4', 'N5', 'L0', 'N12']), ('N4', ['L2', 'L1']), ('N5', ['L3', 'L4', 'L5', 'L6']),
        ('N2', ['M0', 'N6']), ('M0', ['L7', 'N7']), ('N7', ['L8', 'L9']), ('N6', ['U0', 'L10', 'N8']), ('N8', ['L11', 'L12']),
        ('N3', ['N9', 'L13', 'N11']), ('N9', ['L14', 'L15', 'N10']), ('N10', ['L16', 'L17', 'U1']), ('N11', ['L20', 'L18', 'L19']),
        ('N12', ['L21', 'L22', 'N13']), ('N13', ['U2'])]
SMALL_TREE = [('N0', ['b', 'a']), ('a', ['a2', 'a1']), ('b', ['b1']), ('b1', ['b2', 'b3', 'b4'])]


def edge_list(tree, seed):
    rng = np.random.default_rng(seed)
    out = []
    for parent, children in tree:
        for child in children:
            out.append((parent, child, 0.0 if child == 'a1' else round(float(rng.uniform(0.05, 1.5)), 4)))
    return out


def write_inputs():
    os.makedirs(OUT, exist_ok=True)
    for name, tree, seed in (('edges.tsv', TREE, 1), ('edges_small.tsv', SMALL_TREE, 2)):
        with open(os.path.join(OUT, name), 'w') as f:
            for p, c, x in edge_list(tree, seed):
                f.write('%s\t%s\t%r\n' % (p, c, x))
    with open(os.path.join(OUT, 'mrca_to_species.tsv'), 'w') as f:
        for i in range(23):
            f.write('L%d\tS%d\n' % (i, i % 11))
        f.write('M0\tS3\n')
    rng = np.random.default_rng(5)
    values = (rng.random((9, 12)) < np.linspace(0.15, 0.85, 9)[:, None]).astype(np.int64)
    values[0], values[1] = 0, 1
    frame = pd.DataFrame(values, index=['g%d' % g for g in range(9)], columns=['S%d' % s for s in range(12)])
    frame.to_csv(os.path.join(OUT, 'genes_pa.tsv'), sep='\t')


def layout(edges):
    G = cases.graph(nx.DiGraph, edges)
    rounded = []
    ref.round = lambda value, digits: rounded.append(round(value, digits)) or rounded[-1]
    try:
        ax, node_xy = ref.draw_nx_dendrogram(G, cases.ROOT, return_coords=True)
    finally:
        del ref.round
    keys = [child for node in ref.__dict__['__get_bfs_traversal__'](G, cases.ROOT) for child in G[node]]
    assert len(keys) == len(rounded)
    depths = [[cases.ROOT, 0.0]] + [[k, v] for k, v in zip(keys, rounded)]
    return {'depths': depths, 'nodes': list(G), 'node_xy': node_xy.tolist(), 'lines': len(ax.lines), 'arcs': len(ax.patches)}


def main():
    write_inputs()
    G = cases.graph(nx.DiGraph, cases.edges())
    frame, m = cases.table(), cases.mapping()
    out = {'content': {}, 'irregular': {}, 'layout': {}}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        for gene in frame.index:
            out['content'][gene] = cases.pairs(ref.get_node_gene_content(G, frame.loc[gene], m, cases.ROOT))
        single = nx.DiGraph()
        single.add_node('L0')
        out['single_node'] = cases.pairs(ref.get_node_gene_content(single, frame.loc['g1'], m, 'L0'))
        out['boolean'] = cases.pairs(ref.get_node_gene_content(G, frame.loc['g4'].astype(bool), m, cases.ROOT))
        for name in cases.IRREGULAR:
            Gi, fi, mi, root = cases.irregular(name, nx.DiGraph)
            per_gene = {}
            for gene in fi.index:
                try:
                    per_gene[gene] = {'content': cases.pairs(ref.get_node_gene_content(Gi, fi.loc[gene], mi, root))}
                except Exception as e:                    # the type is the record
                    per_gene[gene] = {'raises': type(e).__name__, 'args': [repr(a) for a in e.args]}
            out['irregular'][name] = per_gene
    for key, name in (('tree', 'edges.tsv'), ('small', 'edges_small.tsv')):
        out['layout'][key] = layout(cases.edges(name))
    out['versions'] = {'networkx': nx.__version__, 'numpy': np.__version__, 'pandas': pd.__version__}
    with open(os.path.join(OUT, 'expected.json'), 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    main()
