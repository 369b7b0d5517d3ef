"""pangenomix_amd.weboflife without a device: the single-gene function and the layout against what the reference returned
(tests/golden/weboflife), the table function with ctx=None against the same values column by column, and the device path's
glue -- numbering, heights, chunks, the hand-over of irregular input -- through a stand-in context backed by the model of
tests/tree_content_model.py."""
import warnings

import matplotlib
matplotlib.use('Agg')

import numpy as np                                        # noqa: E402
import pandas as pd                                       # noqa: E402
import pytest                                             # noqa: E402
import scipy.sparse as sp                                 # noqa: E402

import tree_content_model as model                        # noqa: E402
import weboflife_cases as cases                           # noqa: E402
from pangenomix_amd import amr, sparse_utils, synth       # noqa: E402
from pangenomix_amd import weboflife as wol               # noqa: E402

EXPECTED = cases.expected()
FACTORIES = [wol.PhyloGraph, amr.AroGraph]
try:
    import networkx as nx
    FACTORIES.insert(0, nx.DiGraph)
except ImportError:                                       # pragma: no cover
    nx = None


def make(factory, edge_list):
    return cases.graph(factory, edge_list, with_lengths=factory is not amr.AroGraph)


as_frame, lsdf, counts, path_of, check_irregular = cases.as_frame, cases.lsdf, cases.counts, cases.path_of, cases.check_irregular


@pytest.fixture(scope='module')
def golden():
    return cases.edges(), cases.table(), cases.mapping()


# ---- the single-gene function ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('factory', FACTORIES, ids=lambda f: f.__name__)
def test_single_gene_is_the_references(golden, factory):
    edge_list, frame, m = golden
    G = make(factory, edge_list)
    assert len(G) == 41
    for gene in frame.index:
        with pytest.warns(RuntimeWarning, match='invalid value encountered in scalar divide'):
            got = wol.get_node_gene_content(G, frame.loc[gene], m, cases.ROOT)
        assert cases.pairs(got) == EXPECTED['content'][gene]        # the same keys in the same order, the same values
        assert all(type(v) is np.float64 for v in got.values())
    values = dict(EXPECTED['content']['g4'])
    assert values['U0'] is None and values['N13'] is None and values['M0'] in (0.0, 1.0)   # an unmapped leaf, its parent, a mapped one
    assert {'L7', 'N7', 'L8'} <= set(values)                         # the nodes below the mapped node have values of their own
    assert 0.0 < values['N0'] < 1.0


def test_single_gene_on_booleans_and_a_single_node(golden):
    edge_list, frame, m = golden
    G = make(wol.PhyloGraph, edge_list)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        got = wol.get_node_gene_content(G, frame.loc['g4'].astype(bool), m, cases.ROOT)
    assert cases.pairs(got) == EXPECTED['boolean'] == EXPECTED['content']['g4']
    single = wol.PhyloGraph()
    single.add_node('L0')
    assert cases.pairs(wol.get_node_gene_content(single, frame.loc['g1'], m, 'L0')) == EXPECTED['single_node'] == [['L0', 1.0]]


@pytest.mark.parametrize('name', cases.IRREGULAR)
def test_single_gene_raises_what_the_reference_raises(name):
    G, frame, m, root = cases.irregular(name, wol.PhyloGraph)
    raised = set()
    for gene in frame.index:
        want = EXPECTED['irregular'][name][gene]
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)
            if 'raises' in want:
                with pytest.raises(Exception) as e:
                    wol.get_node_gene_content(G, frame.loc[gene], m, root)
                assert type(e.value).__name__ == want['raises'] and [repr(a) for a in e.value.args] == want['args']
                raised.add(want['raises'])
            else:
                assert cases.pairs(wol.get_node_gene_content(G, frame.loc[gene], m, root)) == want['content']
    assert raised == {'two_parents': {'KeyError'}, 'cycle': {'KeyError'}, 'absent_species': {'KeyError'}, 'nan_value': {'ValueError'},
                      'value_two': {'IndexError'}}.get(name, set())


def test_a_missing_root_raises_as_the_traversal_does(golden):
    G = make(wol.PhyloGraph, golden[0])
    with pytest.raises(nx.NetworkXError if nx else KeyError):
        wol.get_node_gene_content(G, golden[1].loc['g1'], golden[2])          # the default root, 'N3623'


@pytest.mark.skipif(nx is None, reason='compares with networkx')
@pytest.mark.parametrize('seed', range(4))
def test_traversals_are_networkxs(seed):
    G, root, _, _ = synth.phylogeny(60, seed, n_genes=1, max_children=5, unmapped_leaves=4)
    H = nx.DiGraph()
    for u in G:
        for v in G[u]:
            H.add_edge(u, v)
    if seed % 2:                                           # no tree any more: nodes with several parents, a cycle
        nodes = list(G)
        for a, b in np.random.default_rng(seed).integers(0, len(nodes), (12, 2)).tolist():
            G.add_edge(nodes[a], nodes[b])
            H.add_edge(nodes[a], nodes[b])
    bfs = list(nx.bfs_successors(H, source=root))
    want = [x[0] for x in bfs] + [s for _, succ in bfs for s in succ if len(H[s]) == 0]
    assert wol.__get_bfs_traversal__(G, root) == want
    assert wol.__get_dfs_preorder__(G, root) == list(nx.dfs_preorder_nodes(H, source=root))


# ---- the table function, host -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ('frame', 'bool frame', 'lsdf'))
@pytest.mark.parametrize('factory', FACTORIES, ids=lambda f: f.__name__)
def test_table_on_the_host_is_the_references_column_by_column(golden, factory, kind):
    edge_list, frame, m = golden
    G = make(factory, edge_list)
    tab = {'frame': frame, 'bool frame': frame.astype(bool), 'lsdf': lsdf(frame)}[kind]
    before = counts()
    with warnings.catch_warnings():
        warnings.simplefilter('error')                    # no warning is emitted
        got = wol.get_node_gene_content_table(G, tab, m, cases.ROOT)
    assert path_of(before) == ['table_host']
    pd.testing.assert_frame_equal(got, as_frame(EXPECTED['content']), check_exact=True)
    assert got.to_numpy().dtype == np.float64 and np.isnan(got.loc['U0']).all() and np.isnan(got.loc['N13']).all()
    some = wol.get_node_gene_content_table(G, tab, m, cases.ROOT, genes=['g7', 'g2'])
    pd.testing.assert_frame_equal(some, as_frame(EXPECTED['content'])[['g7', 'g2']], check_exact=True)
    with pytest.raises(KeyError):
        wol.get_node_gene_content_table(G, tab, m, cases.ROOT, genes=['g7', 'nope'])


@pytest.mark.parametrize('name', cases.IRREGULAR)
def test_table_on_the_host_raises_and_counts_as_the_reference(name):
    check_irregular(name, None, 'table_host')


# ---- the device path through the stand-in -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ('frame', 'bool frame', 'lsdf'))
@pytest.mark.parametrize('factory', FACTORIES, ids=lambda f: f.__name__)
def test_device_path_on_the_golden_tree(golden, factory, kind, monkeypatch):
    edge_list, frame, m = golden
    G = make(factory, edge_list)
    tab = {'frame': frame, 'bool frame': frame.astype(bool), 'lsdf': lsdf(frame)}[kind]
    ctx = model.StandIn()
    before = counts()
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        got = wol.get_node_gene_content_table(G, tab, m, cases.ROOT, ctx=ctx)
    assert path_of(before) == ['table_device'] and ctx.calls == [(9, 41)]
    pd.testing.assert_frame_equal(got, as_frame(EXPECTED['content']), check_exact=True)
    monkeypatch.setattr(wol, '_CHUNK_BYTES', 2 * 4 * 41)  # two genes per call
    ctx = model.StandIn()
    got = wol.get_node_gene_content_table(G, tab, m, cases.ROOT, ctx=ctx)
    assert ctx.calls == [(2, 41)] * 4 + [(1, 41)]
    pd.testing.assert_frame_equal(got, as_frame(EXPECTED['content']), check_exact=True)
    some = wol.get_node_gene_content_table(G, tab, m, cases.ROOT, genes=['g7', 'g2', 'g8'], ctx=ctx)
    pd.testing.assert_frame_equal(some, as_frame(EXPECTED['content'])[['g7', 'g2', 'g8']], check_exact=True)


def test_chunks_fit_the_limit(monkeypatch):
    assert wol._CHUNK_BYTES == 256 << 20
    for n_nodes in (1, 41, 19999, 1 << 20):
        step = wol._chunk_genes(n_nodes)
        assert step % 4 == 0 and 4 * n_nodes * step <= wol._CHUNK_BYTES < 4 * n_nodes * (step + 4)
    monkeypatch.setattr(wol, '_CHUNK_BYTES', 100)
    assert wol._chunk_genes(41) == 1 and wol._chunk_genes(12) == 2 and wol._chunk_genes(5) == 4 and wol._chunk_genes(3) == 8


@pytest.mark.parametrize('seed,n_species,kwargs', [(0, 1, {}), (1, 2, {}), (2, 70, dict(mapped_internal=5, unmapped_leaves=6, unused_species=3)),
                                                   (3, 150, dict(max_children=8, mapped_internal=20, unmapped_leaves=10))])
def test_device_path_on_generated_trees_is_the_host_path(seed, n_species, kwargs, monkeypatch):
    G, root, m, tab = synth.phylogeny(n_species, seed, n_genes=37, **kwargs)
    assert len(m) == n_species + kwargs.get('mapped_internal', 0) and tab.shape == (37, n_species + kwargs.get('unused_species', 0))
    want = wol.get_node_gene_content_table(G, tab, m, root)
    monkeypatch.setattr(wol, '_CHUNK_BYTES', 4 * len(G) * 8)
    before = counts()
    got = wol.get_node_gene_content_table(G, tab, m, root, ctx=model.StandIn())
    assert path_of(before) == ['table_device']
    pd.testing.assert_frame_equal(got, want, check_exact=True)
    dense = pd.DataFrame(tab.values, index=tab.index, columns=tab.columns)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        for gene in list(tab.index[:3]) + [tab.index[-1]]:
            single = wol.get_node_gene_content(G, dense.loc[gene], m, root)
            assert list(single) == list(got.index)
            assert np.array_equal(np.array(list(single.values())), got[gene].to_numpy(), equal_nan=True)


@pytest.mark.parametrize('name', cases.IRREGULAR)
def test_irregular_input_goes_to_the_host(name):
    check_irregular(name, model.StandIn(), 'table_device' if name == 'shared_child_of_mapped' else 'table_host')


def test_duplicate_coordinates_and_refused_sizes_go_to_the_host(golden, monkeypatch):
    edge_list, frame, m = golden
    G = make(wol.PhyloGraph, edge_list)
    tab = lsdf(frame)
    coo = tab.data
    r, c = int(coo.row[0]), int(coo.col[0])                # a stored one a second time: .values reads 2 there
    twice = sp.coo_matrix((np.append(coo.data, 1), (np.append(coo.row, r), np.append(coo.col, c))), shape=coo.shape)
    dup = sparse_utils.LightSparseDataFrame(tab.index, tab.columns, twice)
    for ctx in (None, model.StandIn()):
        before = counts()
        with pytest.raises(IndexError, match='index 2 is out of bounds'):
            wol.get_node_gene_content_table(G, dup, m, cases.ROOT, ctx=ctx)
        assert path_of(before) == ['table_host']
    ctx = model.StandIn()
    monkeypatch.setattr(ctx, 'tree_content_workspace_bytes', lambda *a: 0, raising=False)
    before = counts()
    got = wol.get_node_gene_content_table(G, tab, m, cases.ROOT, ctx=ctx)
    assert path_of(before) == ['table_host'] and ctx.calls == []
    pd.testing.assert_frame_equal(got, as_frame(EXPECTED['content']), check_exact=True)


# ---- the dendrogram -----------------------------------------------------------------------------------------------------------------
LAYOUT_FACTORIES = [f for f in FACTORIES if f is not amr.AroGraph]


@pytest.mark.parametrize('which,file', (('tree', 'edges.tsv'), ('small', 'edges_small.tsv')))
@pytest.mark.parametrize('factory', LAYOUT_FACTORIES, ids=lambda f: f.__name__)
def test_layout_is_the_references(factory, which, file):
    want = EXPECTED['layout'][which]
    G = make(factory, cases.edges(file))
    depths, angles, node_xy = wol.dendrogram_layout(G, cases.ROOT)
    assert list(G) == want['nodes']
    assert [[k, v] for k, v in depths.items()] == want['depths']        # exactly: sums and round(, 8) alone
    # cos / sin may differ in the last bit between numpy builds, nothing else can
    atol = 4 * np.finfo(np.float64).eps * max(depths.values())
    assert np.allclose(node_xy, np.array(want['node_xy']), rtol=0, atol=atol)
    terminals = [n for n in G if len(G[n]) == 0]
    got = sorted(angles[n]['mean'] for n in terminals)
    assert np.allclose(got, np.arange(len(terminals)) * 2 * np.pi / len(terminals), rtol=0, atol=4 * np.finfo(np.float64).eps * 2 * np.pi)
    for n in G:
        kids = [angles[c]['mean'] for c in G[n]]
        if kids:
            assert angles[n] == {'mean': np.mean(kids), 'max': np.max(kids), 'min': np.min(kids)}
        else:
            assert angles[n]['mean'] == angles[n]['max'] == angles[n]['min']


@pytest.mark.parametrize('which,file', (('tree', 'edges.tsv'), ('small', 'edges_small.tsv')))
def test_drawing_has_the_references_lines_and_arcs(which, file):
    import matplotlib.pyplot as plt
    want = EXPECTED['layout'][which]
    G = make(wol.PhyloGraph, cases.edges(file))
    fig, ax = plt.subplots(1, 1)
    try:
        got = wol.draw_nx_dendrogram(G, cases.ROOT, ax=ax)
        assert got is ax and len(ax.lines) == want['lines'] == len(G) - 1 and len(ax.patches) == want['arcs']
        ax2, xy = wol.draw_nx_dendrogram(G, cases.ROOT, node_colors={n: 'red' for n in G}, return_coords=True)
        assert xy.shape == (len(G), 2) and np.array_equal(xy, wol.dendrogram_layout(G, cases.ROOT)[2])
        assert wol.draw_nx_dendrogram(G, cases.ROOT, node_colors='blue', ax=ax) is ax
    finally:
        plt.close('all')
