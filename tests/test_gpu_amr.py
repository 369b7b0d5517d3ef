"""pangenomix_amd.amr with a device context (pgx_graph_reach, pgx_dict_*, pgx_term_scan) against what the
reference returned on the case of tests/golden/amr and against ctx=None in the same process, printed text included; a
seeded generated case in which several terms of one drug match one annotation, compared in process only, where the order of
a set is shared; and every kind of input the device path leaves to the host. Nothing here needs networkx."""
import collections
import shutil

import pandas as pd
import pytest

import amr_cases as cases
from pangenomix_amd import _native, amr, synth

pytestmark = pytest.mark.gpu
EXPECTED = cases.EXPECTED


@pytest.fixture(scope='module')
def own_graph():
    return cases.graph(use_networkx=False)


class counted(object):
    """with counted() as c: ...; c.delta is what AMR_PATH_COUNTS gained"""

    def __enter__(self):
        self.before = collections.Counter(amr.AMR_PATH_COUNTS)
        return self

    def __exit__(self, *exc):
        self.delta = dict(collections.Counter(amr.AMR_PATH_COUNTS) - self.before)


@pytest.mark.parametrize('lengths', (False, True))
def test_build_resistome_equals_the_reference_and_the_host(lengths, own_graph, gpu_ctx, capsys):
    G = own_graph[0]
    with counted() as c:
        (rgi_d, aro_d), printed_d = cases.resistome(capsys, G, ctx=gpu_ctx, return_path_lengths=lengths)
    assert c.delta == {'resistome_device': 1}
    (rgi_h, aro_h), printed_h = cases.resistome(capsys, G, return_path_lengths=lengths)
    assert printed_d == printed_h == EXPECTED['resistome_stdout']
    pd.testing.assert_frame_equal(aro_d, cases.recorded_frame('df_aro_lengths.tsv' if lengths else 'df_aro.tsv'))
    pd.testing.assert_frame_equal(aro_d, aro_h)
    pd.testing.assert_frame_equal(rgi_d, rgi_h)


def test_probable_hits_equal_the_reference_and_the_host(own_graph, gpu_ctx, capsys):
    G, aro_names = own_graph
    df_aro = cases.recorded_frame('df_aro.tsv')
    with counted() as c:
        prob_d, terms_d, printed_d = cases.probable(capsys, df_aro, G, aro_names, ctx=gpu_ctx)
    assert c.delta == {'class_terms_device': 1, 'screen_device': 1}
    prob_h, terms_h, printed_h = cases.probable(capsys, df_aro, G, aro_names)
    assert printed_d == printed_h and {k: sorted(v) for k, v in terms_d.items()} == EXPECTED['search_terms']
    cases.assert_prob_equal(prob_d, cases.recorded_frame('df_prob.tsv'))
    pd.testing.assert_frame_equal(prob_d, prob_h)
    for kwargs in ({'G_aro': None}, {'check_drug_mentions': False}, {'exclude': []}, {'manual_annots': {}, 'drug_to_aro': {}},
                   {'exclude': ['Class A beta-lactamase (EC 3.5.2.6)', 'TEM family']}, {'manual_annots': {'vancomycin': ['']}}):
        with counted() as c:
            got = cases.probable(capsys, df_aro, G, aro_names, ctx=gpu_ctx, **kwargs)
        assert c.delta.get('screen_device') == 1 and 'screen_host' not in c.delta, kwargs
        want = cases.probable(capsys, df_aro, G, aro_names, **kwargs)
        pd.testing.assert_frame_equal(got[0], want[0])
        assert got[2] == want[2]


@pytest.fixture(scope='module')
def generated(tmp_path_factory):
    """~300 ontology terms, 200 hits, 12 drugs, 2,000 annotation lines"""
    out = tmp_path_factory.mktemp('amr_generated')
    case = synth.write_amr_case(str(out), amr.DRUG_CLASS_AROS, n_terms=300, n_hits=200, n_drugs=12, n_lines=2000, seed=2026)
    old, amr.USE_NETWORKX = amr.USE_NETWORKX, False
    try:
        case['G'], case['aro_names'] = amr.construct_aro_to_drug_network(case['obo'])
    finally:
        amr.USE_NETWORKX = old
    return case


def test_generated_case_equals_the_host_in_process(generated, gpu_ctx, capsys):
    g = generated
    G, aro_names = g['G'], g['aro_names']
    for lengths in (False, True):
        with counted() as c:
            (rgi_d, aro_d), printed_d = cases.resistome(capsys, G, ctx=gpu_ctx, rgi=g['rgi'], drugs=g['drugs'],
                                                        return_path_lengths=lengths)
        assert c.delta == {'resistome_device': 1}
        (rgi_h, aro_h), printed_h = cases.resistome(capsys, G, rgi=g['rgi'], drugs=g['drugs'], return_path_lengths=lengths)
        assert printed_d == printed_h and printed_d.count('Duplicate hit:') >= 3
        pd.testing.assert_frame_equal(aro_d, aro_h)
    assert aro_d.iloc[:, 1:].notna().any().sum() >= 6 and (aro_d.iloc[:, 1:] > 3).any().any() and len(aro_d) > 100
    kwargs = dict(annotations=g['annotations'], drug_to_aro=g['drug_to_aro'], manual_annots=g['manual_annots'])
    with counted() as c:
        prob_d, terms, printed_d = cases.probable(capsys, aro_d, G, aro_names, ctx=gpu_ctx, **kwargs)
    assert c.delta == {'class_terms_device': 1, 'screen_device': 1}
    prob_h, _, printed_h = cases.probable(capsys, aro_d, G, aro_names, **kwargs)
    assert printed_d == printed_h
    pd.testing.assert_frame_equal(prob_d, prob_h)
    assert len(prob_d) > 500 and prob_d['card_hits'].notna().any() and prob_d['card_hits'].isna().any()
    # several terms of one drug match one annotation: which one is reported is the set's order, shared in process
    several = 0
    for annot, drug in set(zip(prob_d['shared_annot'], prob_d['drug'])):
        several += len({t for t in terms[drug] if t.lower() in annot.lower()}) > 1
    assert several >= 3


def irregular_files(tmp_path):
    """name -> an annotations file the device path must leave to the host loop"""
    lines = open(cases.ANNOTATIONS, 'rb').read().split(b'\n')[:-1]
    variants = {
        'non_ascii': lines[:3] + [b'Eco_C30A0\tBeta-lactamase \xc3\x9f'] + lines[3:],
        'crlf': [x + b'\r' for x in lines],
        'trailing_space': lines[:5] + [lines[5] + b' '] + lines[6:],
        'leading_tab': lines[:2] + [b'\tEco_C31A0\tTEM family'] + lines[2:],
        'trailing_tab': lines[:-1] + [lines[-1] + b'\t'],
        'blank_line': lines[:4] + [b''] + lines[4:],
    }
    paths = {}
    for name, body in variants.items():
        paths[name] = str(tmp_path / (name + '.tsv'))
        with open(paths[name], 'wb') as f:
            f.write(b'\n'.join(body) + b'\n')
    return paths


def test_irregular_input_lands_on_the_host_path_with_equal_output(own_graph, gpu_ctx, capsys, tmp_path):
    G, aro_names = own_graph
    df_aro = cases.recorded_frame('df_aro.tsv')
    for name, path in sorted(irregular_files(tmp_path).items()):
        with counted() as c:
            got = cases.probable(capsys, df_aro, G, aro_names, ctx=gpu_ctx, annotations=path)
        assert c.delta == {'class_terms_device': 1, 'screen_host': 1}, name
        want = cases.probable(capsys, df_aro, G, aro_names, annotations=path)
        pd.testing.assert_frame_equal(got[0], want[0])
        assert got[2] == want[2] and len(got[0]) >= 30, name
    # term sets beyond what the kernel holds, and a term that is not ASCII text
    many = {'vancomycin': ['term %d' % i for i in range(_native.TERM_MAX_TERMS)]}
    long_ones = {'vancomycin': ['x' * 300 + str(i) for i in range(_native.TERM_MAX_BYTES // 300 + 1)]}
    for manual, path_taken in ((many, 'screen_host'), (long_ones, 'screen_host'), ({'vancomycin': ['ß-lactamase']}, 'screen_host'),
                               ({'vancomycin': ['term %d' % i for i in range(400)]}, 'screen_device')):
        with counted() as c:
            got = cases.probable(capsys, df_aro, G, aro_names, ctx=gpu_ctx, manual_annots=manual)
        assert c.delta == {'class_terms_device': 1, path_taken: 1}
        want = cases.probable(capsys, df_aro, G, aro_names, manual_annots=manual)
        pd.testing.assert_frame_equal(got[0], want[0])
        assert got[2] == want[2]


def test_nodes_that_are_missing_raise_as_on_the_host(own_graph, gpu_ctx, capsys, tmp_path):
    G, aro_names = own_graph
    rgi = tmp_path / 'rgi.txt'
    shutil.copy(cases.RGI, rgi)
    with open(rgi, 'a') as f:
        f.write('Eco_C40A0\tc9\tStrict\tnothing\t1234567\n')
    for kwargs, message in (({'rgi': str(rgi)}, 'Source ARO:1234567 is not in G'),
                            ({'drugs': dict(cases.DRUGS, nothing='ARO:7777777')}, 'Target ARO:7777777 is not in G')):
        printed = []
        for ctx in (gpu_ctx, None):
            capsys.readouterr()
            with counted() as c:
                with pytest.raises(amr.NodeNotFound, match=message):
                    amr.build_resistome(kwargs.get('rgi', cases.RGI), kwargs.get('drugs', cases.DRUGS), G, ctx=ctx)
            assert c.delta == {'resistome_host': 1}
            printed.append(capsys.readouterr().out)
        assert printed[0] == printed[1]
    # a drug whose name maps to an ARO that is no node: the class terms are the host's, and raise what the host raises
    names = dict(aro_names, **{'ARO:7777777': 'vancomycin'})
    df_aro = cases.recorded_frame('df_aro.tsv')
    for ctx in (gpu_ctx, None):
        with counted() as c:
            with pytest.raises(amr.NodeNotFound, match='Target ARO:7777777 is not in G'):
                cases.probable(capsys, df_aro, G, names, ctx=ctx)
        assert c.delta == {'class_terms_host': 1}


def test_empty_tables_and_no_drugs(own_graph, gpu_ctx, capsys, tmp_path):
    G = own_graph[0]
    rgi = tmp_path / 'rgi.txt'
    rgi.write_text(open(cases.RGI).readline())
    for kwargs in ({'rgi': str(rgi)}, {'drugs': {}}):
        (_, got), _ = cases.resistome(capsys, G, ctx=gpu_ctx, **kwargs)
        (_, want), _ = cases.resistome(capsys, G, **kwargs)
        pd.testing.assert_frame_equal(got, want)
