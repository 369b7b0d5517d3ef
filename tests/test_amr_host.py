"""pangenomix_amd.amr with ctx=None (the reference's loops restated) against what the reference returned and printed on the
case of tests/golden/amr, and the parts the reference cannot run any more against hand-written expectations. Frames are
compared with assert_frame_equal: values, dtypes, index and column order."""
import numpy as np
import pandas as pd
import pytest

import amr_cases as cases
import reach_model
import terms_model
from pangenomix_amd import amr

EXPECTED = cases.EXPECTED


@pytest.fixture(scope='module')
def own_graph():
    return cases.graph(use_networkx=False)


@pytest.mark.parametrize('use_networkx', (False, None))
def test_the_graph_has_the_references_nodes_and_edges_in_its_order(use_networkx):
    if use_networkx is None:
        nx = pytest.importorskip('networkx')
    G, aro_names = cases.graph(use_networkx)
    assert isinstance(G, amr.AroGraph) if use_networkx is False else isinstance(G, nx.DiGraph)
    assert list(G.nodes) == EXPECTED['nodes'] and [list(e) for e in G.edges] == EXPECTED['edges']
    assert aro_names == EXPECTED['aro_names'] and list(aro_names) == list(EXPECTED['aro_names'])
    assert 'ARO:1000001' not in G and 'ARO:9999999' in G and 'ARO:8888888' not in G and len(G) == len(EXPECTED['nodes'])
    assert sorted(G.successors('ARO:3000188')) == ['ARO:3004024']               # has_part is reversed
    assert not any('ARO:3003000' == u and v == 'ARO:3000007' for u, v in G.edges)   # participates_in is ignored


def test_aro_graph_methods():
    G = amr.AroGraph()
    G.add_edge('b', 'a')
    G.add_node('c')
    G.add_edge('a', 'b')
    G.add_edge('b', 'a')                                                         # again: still one edge
    G.add_edge('a', 'a')
    G.add_edge('c', 'a')
    assert G.nodes == ['b', 'a', 'c'] and G.edges == [('b', 'a'), ('a', 'b'), ('a', 'a'), ('c', 'a')] and len(G) == 3
    assert list(G.successors('a')) == ['b', 'a'] and 'a' in G and 'z' not in G and [] not in G
    G.remove_node('a')
    assert G.nodes == ['b', 'c'] and G.edges == []
    with pytest.raises(amr.AroGraphError):
        G.remove_node('a')


@pytest.mark.parametrize('lengths', (False, True))
def test_build_resistome_equals_the_reference(lengths, own_graph, capsys):
    (df_rgi, df_aro), printed = cases.resistome(capsys, own_graph[0], return_path_lengths=lengths)
    assert printed == EXPECTED['resistome_stdout'] == 'Duplicate hit: Eco_C10A0\n'
    pd.testing.assert_frame_equal(df_aro, cases.recorded_frame('df_aro_lengths.tsv' if lengths else 'df_aro.tsv'))
    assert df_aro.columns.tolist() == ['ARO'] + sorted(cases.DRUGS) and df_aro['vancomycin'].isna().all()
    assert df_aro.index.tolist()[0] == 'Eco_C10A0' and df_aro.loc['Eco_C10A0', 'ARO'] == 3001878   # later ARO, first place
    raw = pd.read_csv(cases.RGI, sep='\t')
    pd.testing.assert_frame_equal(df_rgi, raw[raw.Cut_Off != 'Loose'])
    (df_all, _), _ = cases.resistome(capsys, own_graph[0], skip_loose=False)
    pd.testing.assert_frame_equal(df_all, raw)


def test_a_hit_or_a_drug_that_is_no_node_raises_and_names_it(own_graph, capsys, tmp_path):
    G = own_graph[0]
    rgi = tmp_path / 'rgi.txt'
    rgi.write_text('ORF_ID\tCut_Off\tARO\nEco_C1A0\tStrict\t3000873\nEco_C1A0\tStrict\t1234567\n')
    with pytest.raises(amr.NodeNotFound, match='Source ARO:1234567 is not in G'):
        amr.build_resistome(str(rgi), cases.DRUGS, G)
    assert capsys.readouterr().out == 'Duplicate hit: Eco_C1A0\n'               # raised after the print of that row
    with pytest.raises(amr.NodeNotFound, match='Target ARO:7777777 is not in G'):
        amr.build_resistome(cases.RGI, {'ampicillin': 'ARO:3000637', 'nothing': 'ARO:7777777'}, G)
    _, df_aro = amr.build_resistome(str(rgi), {}, G)                             # without drugs nothing is looked up
    assert df_aro.columns.tolist() == ['ARO'] and df_aro['ARO'].tolist() == [1234567]


def test_probable_hits_equal_the_reference(own_graph, capsys):
    G, aro_names = own_graph
    df_aro = cases.recorded_frame('df_aro.tsv')
    df_prob, terms, printed = cases.probable(capsys, df_aro, G, aro_names)
    assert {k: sorted(v) for k, v in terms.items()} == EXPECTED['search_terms'] and printed.count('\n') == 1
    cases.assert_prob_equal(df_prob, cases.recorded_frame('df_prob.tsv'))
    assert df_prob.columns.tolist() == ['feature', 'drug', 'shared_annot', 'card_hits', 'related_aros', 'shared_gene']
    assert 'hypothetical protein' not in set(df_prob['shared_annot'])
    same, _, _ = cases.probable(capsys, df_aro, G, aro_names, ignore_case=False)   # the parameter changes nothing
    pd.testing.assert_frame_equal(same, df_prob)
    # without the graph: no class terms; without drug mentions: only the exact annotations and the two dictionaries
    no_graph, terms, _ = cases.probable(capsys, df_aro, None, aro_names)
    assert terms['ampicillin'] == {'ampicillin'} and terms['gentamicin'] == {'gentamicin', 'AAC(3)'}
    assert not (no_graph['related_aros'] == 'beta-lactam').any() and (no_graph['related_aros'] == 'gyrase').any()
    exact, terms, _ = cases.probable(capsys, df_aro, G, aro_names, check_drug_mentions=False)
    assert terms == {'gentamicin': {'AAC(3)'}, 'ciprofloxacin': {'gyrase'}}
    assert exact['card_hits'].notna().sum() == df_prob['card_hits'].notna().sum() and exact['card_hits'].isna().sum() == 2


def test_add_probable_hits():
    nan = np.nan
    df_aro = pd.DataFrame({'ARO': [3000873, 3001878], 'ampicillin': [1.0, nan], 'gentamicin': [nan, nan]}, index=['E_C1A0', 'E_C2A0'])
    df_prob = pd.DataFrame(
        columns=['feature', 'drug', 'shared_annot', 'card_hits', 'related_aros', 'shared_gene', 'org'],
        data=[('E_C3A0', 'ampicillin', 'Class A beta-lactamase', 'E_C1A0', '3000873', False, 'eco'),
              ('E_C4A0', 'ampicillin', 'Class A beta-lactamase', 'E_C1A0;E_C2A0', '3000873;3001878', False, 'eco'),
              ('E_C5A0', 'gentamicin', 'gentamicin acetyltransferase', nan, 'gentamicin', False, 'eco'),
              ('E_C6A0', 'colistin', 'colistin resistance', nan, 'colistin', False, 'eco'),          # not a drug of df_aro
              ('K_C7A0', 'ampicillin', 'Class A beta-lactamase', 'K_C1A0', '3000873', False, 'kpn'),  # another organism
              ('E_C8A0', 'gentamicin', 'AAC(3)', nan, nan, False, 'eco')])
    want = pd.DataFrame({'ARO': [3000873, 3001878, '*3000873', '*3000873;3001878', 'Inferred', 'Inferred'],
                         'ampicillin': [1.0, nan, 1.0, 1.0, nan, nan], 'gentamicin': [nan, nan, nan, nan, 1.0, 1.0]},
                        index=['E_C1A0', 'E_C2A0', 'E_C3A0', 'E_C4A0', 'E_C5A0', 'E_C8A0'])
    before = df_aro.copy(deep=True)
    pd.testing.assert_frame_equal(amr.add_probable_hits(df_aro, df_prob, 'eco'), want)
    pd.testing.assert_frame_equal(df_aro, before)
    pd.testing.assert_frame_equal(amr.add_probable_hits(df_aro, df_prob, 'nobody'), df_aro)


def test_add_probable_hits_prints_its_additions(capsys):
    df_aro = pd.DataFrame({'ARO': [1], 'ampicillin': [1.0]}, index=['E_C1A0'])
    df_prob = pd.DataFrame(columns=['feature', 'drug', 'shared_annot', 'card_hits', 'related_aros', 'shared_gene', 'org'],
                           data=[('E_C3A0', 'ampicillin', 'penam hydrolase', np.nan, 'penam', False, 'eco')])
    amr.add_probable_hits(df_aro, df_prob, 'eco', print_additions=True)
    assert capsys.readouterr().out == 'E_C3A0 ampicillin penam hydrolase\n'


def test_both_kinds_of_graph_give_equal_results(capsys):
    pytest.importorskip('networkx')
    (G_own, names_own), (G_nx, names_nx) = cases.graph(False), cases.graph(None)
    assert names_own == names_nx
    for lengths in (False, True):
        (_, a), _ = cases.resistome(capsys, G_own, return_path_lengths=lengths)
        (_, b), _ = cases.resistome(capsys, G_nx, return_path_lengths=lengths)
        pd.testing.assert_frame_equal(a, b)
    p_own, t_own, _ = cases.probable(capsys, a, G_own, names_own)
    p_nx, t_nx, _ = cases.probable(capsys, a, G_nx, names_nx)
    assert t_own == t_nx
    pd.testing.assert_frame_equal(p_own, p_nx)


def test_the_models_agree_with_networkx_on_random_graphs():
    nx = pytest.importorskip('networkx')
    for seed in range(3):
        rng = np.random.default_rng(seed)
        n = 200
        edges = list(zip(rng.integers(0, n, 300).tolist(), rng.integers(0, n, 300).tolist()))
        G = nx.DiGraph()
        G.add_nodes_from(range(n))
        G.add_edges_from(edges)
        off, succ = reach_model.csr(n, edges)
        sources, targets = rng.integers(0, n, 15).tolist(), rng.integers(0, n, 15).tolist()
        want = np.array([[len(nx.shortest_path(G, s, t)) if nx.has_path(G, s, t) else 0 for t in targets] for s in sources])
        assert np.array_equal(reach_model.lengths(off, succ, targets, sources), want) and (want > 2).any() and (want == 0).any()
        host = amr._HostPaths(G)
        assert [[host.nodes_on_path(s, t) for t in targets] for s in sources] == want.tolist()
        assert reach_model.rounds(off, succ, targets) == 1 + max(
            d for t in set(targets) for d in nx.shortest_path_length(G, target=t).values())


def test_the_term_model_is_pythons_in_on_lowered_ascii_text():
    strings = ['Class A Beta-Lactamase', '', '[@`{', 'AZ az']
    terms = ['beta-lactam', 'BETA', '', '{@', '[@', 'Z A', 'lactamases']
    text, start, length = terms_model.windows([s.encode() for s in strings])
    got = terms_model.masks(text, start, length, [t.encode() for t in terms], terms_model.FOLD)
    for i, s in enumerate(strings):
        for t, term in enumerate(terms):
            assert bool((int(got[i, 0]) >> t) & 1) == (term.lower() in s.lower()), (s, term)
    assert terms_model.masks(text, start, length, [t.encode() for t in terms], 0)[:, 0].tolist() == [0b100, 0b100, 0b10100, 0b100]
    # bytes outside A-Z are never folded: 0xC1 / 0xE1 differ by 0x20 as 'A' / 'a' do
    text, start, length = terms_model.windows([b'\xc1@'])
    assert terms_model.masks(text, start, length, [b'\xe1', b'\xc1', b'`'], terms_model.FOLD)[0, 0] == 0b010
