"""TEST INFRASTRUCTURE for weboflife: the golden fixture (tests/golden/weboflife, written by make_golden_weboflife.py from the
reference), graphs of every accepted kind from its edge list, and the irregular inputs, each a change of the fixture. The
golden maker uses the first half, which does not import the package; the checks at the end import it where they need it."""
import json
import os

import numpy as np
import pandas as pd

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'weboflife')
ROOT = 'N0'


def edges(name='edges.tsv'):
    """[(parent, child, length)] in insertion order"""
    with open(os.path.join(GOLDEN, name)) as f:
        return [(p, c, float(x)) for p, c, x in (line.rstrip('\n').split('\t') for line in f if line.strip())]


def mapping():
    with open(os.path.join(GOLDEN, 'mrca_to_species.tsv')) as f:
        return dict(line.rstrip('\n').split('\t') for line in f if line.strip())


def table():
    """the gene x species frame of 0 / 1"""
    return pd.read_csv(os.path.join(GOLDEN, 'genes_pa.tsv'), sep='\t', index_col=0)


def expected():
    with open(os.path.join(GOLDEN, 'expected.json')) as f:
        return json.load(f)


def graph(factory, edge_list, with_lengths=True):
    """factory(): an empty nx.DiGraph, weboflife.PhyloGraph or amr.AroGraph (the last takes no attributes)"""
    G = factory()
    for p, c, x in edge_list:
        if with_lengths:
            G.add_edge(p, c, len=x)
        else:
            G.add_edge(p, c)
    return G


def pairs(content):
    """a dict of node -> value as ordered pairs, nan as None (what expected.json holds)"""
    return [[k, None if v != v else float(v)] for k, v in content.items()]


SMALL = {'two_parents': [('R', 'A'), ('R', 'B'), ('A', 'x'), ('B', 'x')],
         'two_parents_listed': [('R', 'A'), ('R', 'B'), ('A', 'x'), ('B', 'x'), ('B', 'y')],
         'cycle': [('R', 'A'), ('A', 'R'), ('A', 'x')]}
IRREGULAR = ('two_parents', 'two_parents_listed', 'cycle', 'absent_species', 'nan_value', 'value_two', 'value_minus_one',
             'value_half', 'shared_child_of_mapped')


def irregular(name, factory):
    """(G, frame, mrca_to_species, root) of one irregular input"""
    frame, m = table().astype(np.float64), mapping()
    if name in SMALL:
        G = graph(factory, [(p, c, 1.0) for p, c in SMALL[name]], with_lengths=False)
        return G, frame, {'x': 'S0', 'y': 'S1'}, 'R'
    edge_list = edges()
    if name == 'absent_species':
        m['L0'] = 'S99'
    elif name == 'nan_value':
        frame.loc['g3', 'S4'] = np.nan
    elif name == 'value_two':
        frame.loc['g3', 'S4'] = 2
    elif name == 'value_minus_one':                       # indexes the last counter: counts as present
        frame.loc['g3', 'S4'] = -1
    elif name == 'value_half':                            # int() truncates: counts as absent
        frame.loc['g5', 'S2'] = 0.5
    elif name == 'shared_child_of_mapped':                # a second parent that is mapped: its children are not consulted
        edge_list = edge_list + [('M0', 'L1', 0.5)]
    else:
        raise KeyError(name)
    return graph(factory, edge_list, with_lengths=False), frame, m, ROOT


# ---- what the host and the GPU tests of the table function share (the package is imported where it is needed) ---------------------
def as_frame(per_gene):
    """the recorded dicts of several genes as the frame the table function returns"""
    genes = list(per_gene)
    nodes = [k for k, _ in per_gene[genes[0]]]
    data = {g: [np.nan if v is None else v for _, v in per_gene[g]] for g in genes}
    return pd.DataFrame(data, index=pd.Index(nodes), columns=genes, dtype=np.float64)


def lsdf(frame):
    import scipy.sparse as sp
    from pangenomix_amd import sparse_utils
    return sparse_utils.LightSparseDataFrame(np.array(frame.index, dtype=object), np.array(frame.columns, dtype=object),
                                             sp.coo_matrix(frame.to_numpy()))


def counts():
    from pangenomix_amd import weboflife as wol
    return dict(wol.WEBOFLIFE_PATH_COUNTS)


def path_of(before):
    after = counts()
    return [k for k in after if after[k] != before.get(k, 0)]


def check_irregular(name, ctx, want_path):
    """the table function on one irregular input, against the reference's record gene by gene"""
    import pytest
    from pangenomix_amd import weboflife as wol
    G, frame, m, root = irregular(name, wol.PhyloGraph)
    record = expected()['irregular'][name]
    raising = [g for g in frame.index if 'raises' in record[g]]
    before = counts()
    if raising:
        with pytest.raises(Exception) as e:
            wol.get_node_gene_content_table(G, frame, m, root, ctx=ctx)
        assert type(e.value).__name__ == record[raising[0]]['raises']
        assert [repr(a) for a in e.value.args] == record[raising[0]]['args']
        keep = [g for g in frame.index if g not in raising]
        if len(raising) == len(frame.index):
            return
        assert path_of(before) == ['table_host']
        before = counts()
        got = wol.get_node_gene_content_table(G, frame, m, root, genes=keep, ctx=ctx)     # without the rows that raise
        want = as_frame({g: record[g]['content'] for g in keep})
        assert path_of(before) == (['table_device'] if ctx is not None else ['table_host'])
    else:
        got = wol.get_node_gene_content_table(G, frame, m, root, ctx=ctx)
        want = as_frame({g: record[g]['content'] for g in frame.index})
        assert path_of(before) == [want_path]
    pd.testing.assert_frame_equal(got, want, check_exact=True)
