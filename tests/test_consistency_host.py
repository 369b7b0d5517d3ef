"""Host side of the gene-table / allele-table checks (pangenomix_amd/pangenome.py validate_gene_table,
validate_gene_table_dense, extract_dominant_alleles), without a GPU: the numpy model of the device pass
(tests/allele_runs_model.py) against what the reference printed for every fixture of tests/golden/consistency, the
construction of the runs for both grouping rules, the small name helpers, and the parser of the recorded stdout."""
import glob
import os

import numpy as np
import pytest

import allele_runs_model as model
from pangenomix_amd import pangenome

CASES = sorted(glob.glob(os.path.join(model.GOLDEN, '*.npz')))
ids = [os.path.basename(p)[:-4] for p in CASES]


def test_the_fixtures_cover_the_cases():
    assert ids == ['all_absent_gene', 'allele_gene_missing', 'consistent', 'count_tie', 'explicit_zero',
                   'flipped_gene_cells', 'gene_without_alleles', 'lexicographic_clusters', 'recurring_gene']


@pytest.mark.parametrize('path', CASES, ids=ids)
def test_model_gives_the_counts_the_reference_printed(path):
    case = model.load_case(path)
    (G, genes, _), (A, alleles, _) = case['genes'], case['alleles']
    # validate_gene_table: present = not NaN, alleles grouped by name
    names, run_start, gene_of_run, order = model.runs_by_name(genes, alleles)
    out = model.runs(~np.isnan(A)[order], run_start, ~np.isnan(G), gene_of_run)
    lines, count = model.parse_validate_stdout(case['stdout_validate'])
    assert int(out['diff_per_genome'].sum()) == count
    sets = [x for x in lines if isinstance(x, frozenset)]
    assert sets == [frozenset(names[r] for r in np.flatnonzero(out['diff'][:, j])) for j in range(A.shape[1])
                    if out['diff_per_genome'][j]]
    # validate_gene_table_dense: present = 1, runs in table order
    run_names, run_start = model.runs_in_order(alleles)
    if case['dense_raises']:
        assert any(n not in genes for n in run_names)
    else:
        out = model.runs(A == 1, run_start, G == 1, [genes.index(n) for n in run_names])
        _, count, printed = model.parse_dense_stdout(case['stdout_dense'])
        bad = np.flatnonzero(out['diff_per_run'])
        assert bad.size == count
        assert printed == [run_names[min(r + 1, len(run_names) - 1)] for r in bad]
    # extract_dominant_alleles
    run_names, run_start = model.runs_in_order(alleles, pangenome._gene_name_of_allele)
    out = model.runs(A == 1, run_start)
    kept = np.flatnonzero(out['total'] > 0)
    want = case['dominant']
    assert [run_names[r] for r in kept] == want['gene']
    assert [alleles[i] for i in out['best_allele'][kept]] == want['dominant_allele']
    assert np.array_equal(out['total'][kept].astype(np.float64), want['gene_count'])
    assert np.array_equal(out['best_count'][kept].astype(np.float64), want['allele_count'])


@pytest.mark.parametrize('as_lsdf', (False, True), ids=('frames', 'lsdf'))
@pytest.mark.parametrize('path', CASES, ids=ids)
def test_python_layer_on_the_model(path, as_lsdf, tmp_path):
    """Everything but the kernels: labels -> runs -> (model) -> printed lines, counts, df_dominant, FASTA."""
    model.check_python_functions(model.load_case(path), model.ModelContext(), str(tmp_path), as_lsdf)


def test_the_explicit_zero_separates_the_two_validators():
    case = model.load_case(os.path.join(model.GOLDEN, 'explicit_zero.npz'))
    assert model.has_stored_zero(case)
    assert model.parse_validate_stdout(case['stdout_validate'])[1] == 2
    assert model.parse_dense_stdout(case['stdout_dense'])[1] == 0


def test_runs_by_name_for_any_order_of_the_alleles():
    rng = np.random.default_rng(7)
    genes = ['T_C%d' % c for c in (1, 10, 100, 2, 7)]
    alleles = ['T_C%dA%d' % (c, m) for c in (1, 10, 2, 55, 3) for m in range(3)] + ['noallele', 'T_C55A9']
    for _ in range(20):
        shuffled = [alleles[i] for i in rng.permutation(len(alleles))]
        names, run_start, gene_of_run, new_row = pangenome._runs_by_name(genes, pangenome._genes_of_alleles(shuffled))
        w_names, w_start, w_gene, w_order = model.runs_by_name(genes, shuffled)
        assert names.tolist() == w_names and run_start.tolist() == w_start.tolist() and gene_of_run.tolist() == w_gene.tolist()
        assert run_start.dtype == np.uint32 and gene_of_run.dtype == np.int32
        assert np.array_equal(np.argsort(new_row), w_order)
        assert [pangenome.__get_gene_from_allele__(shuffled[i]) for i in w_order] == \
            [names[r] for r in range(len(names)) for _ in range(run_start[r + 1] - run_start[r])]
    # genes 100 and 7 have no allele: empty runs; 55, 3 and '' (a label without 'A') occur only among the alleles
    names, run_start, gene_of_run, _ = pangenome._runs_by_name(genes, pangenome._genes_of_alleles(alleles))
    assert names.tolist() == genes + ['T_C55', 'T_C3', '']
    assert np.diff(run_start.astype(np.int64)).tolist() == [3, 3, 0, 3, 0, 4, 3, 1]
    assert gene_of_run.tolist() == [0, 1, 2, 3, 4, -1, -1, -1]
    with pytest.raises(ValueError, match='repeated'):
        pangenome._runs_by_name(['a', 'a'], np.array(['a']))
    names, run_start, gene_of_run, new_row = pangenome._runs_by_name([], np.array([], dtype=str))
    assert names.size == 0 and run_start.tolist() == [0] and gene_of_run.size == 0 and new_row.size == 0


def test_runs_in_table_order_let_a_gene_recur():
    alleles = ['T_C1A0', 'T_C1A1', 'T_C2A0', 'T_C1A2', 'T_C10A0', 'T_C10A1']
    names, run_start = pangenome._runs_in_order(pangenome._genes_of_alleles(alleles))
    assert names.tolist() == ['T_C1', 'T_C2', 'T_C1', 'T_C10'] and run_start.tolist() == [0, 2, 3, 4, 6]
    w_names, w_start = model.runs_in_order(alleles)
    assert names.tolist() == w_names and run_start.tolist() == w_start.tolist()
    names, run_start = pangenome._runs_in_order([])
    assert names.size == 0 and run_start.tolist() == [0]
    assert pangenome._gene_name_of_allele('T_x_C012A3') == 'T_x_C12'      # (the number is parsed, unlike the split on 'A')


def test_name_helpers_on_the_docstring_examples():
    assert pangenome.breakdown_feature_name('EsC_A123U56') == ('EsC', 'A', 123, 'U', 56)
    assert pangenome.breakdown_feature_name('PsA_T789') == ('PsA', 'T', 789, None, None)
    assert pangenome.breakdown_feature_name('a_b_C4D0') == ('a_b', 'C', 4, 'D', 0)
    assert pangenome.trim_variant('EsC_C123A56') == 'EsC_C123'
    assert pangenome.trim_variant('EsC_C123U5') == 'EsC_C123'
    assert pangenome.trim_variant('1234') == '1234'
    assert pangenome.trim_variant('A12') == 'A12'                         # the first character is never looked at
    assert pangenome.load_feature_table(5) == 5 and pangenome.load_feature_table('table.txt') == 'table.txt'


def test_load_feature_table_reads_csv_and_pickle(tmp_path):
    import pandas as pd
    df = pd.DataFrame([[1.0, np.nan], [np.nan, 1.0]], index=['T_C0A0', 'T_C1A0'], columns=['g0', 'g1'])
    df.to_csv(str(tmp_path / 't.csv'))
    df.to_pickle(str(tmp_path / 't.pickle'))
    for name in ('t.csv', 't.pickle'):
        pd.testing.assert_frame_equal(pangenome.load_feature_table(str(tmp_path / name)), df)


def test_values_other_than_the_rule_allows_are_refused():
    import pandas as pd
    import scipy.sparse
    from pangenomix_amd import sparse_utils
    two = pd.DataFrame([[2.0, np.nan]], index=['T_C0A0'], columns=['g0', 'g1'])
    genes = pd.DataFrame([[1.0, np.nan]], index=['T_C0'], columns=['g0', 'g1'])
    ctx = model.ModelContext()
    with pytest.raises(ValueError, match='binary'):
        pangenome.validate_gene_table_dense(genes, two, ctx=ctx)
    with pytest.raises(ValueError, match='binary'):
        pangenome.extract_dominant_alleles(two, 'unused', 'unused', ctx=ctx)
    zero = sparse_utils.LightSparseDataFrame(['T_C0A0'], ['g0', 'g1'],
                                             scipy.sparse.coo_matrix((np.array([1, 0]), ([0, 0], [0, 1])), shape=(1, 2)))
    with pytest.raises(ValueError, match='stored zeros'):
        pangenome.validate_gene_table(genes, zero, ctx=ctx)


def test_stdout_parser():
    text = ("Validating gene clusters...\n1 Testing g0\n\tInconsistent: {'T_C2', 'T_C10'}\n2 Testing g1\n"
            "Gene Table Inconsistencies: 2\n")
    lines, count = model.parse_validate_stdout(text)
    assert count == 2
    assert lines == ['Validating gene clusters...', '1 Testing g0', frozenset(['T_C10', 'T_C2']), '2 Testing g1',
                     'Gene Table Inconsistencies: 2']
    assert model.parse_validate_stdout(text.replace("'T_C2', 'T_C10'", "'T_C10', 'T_C2'"))[0] == lines
    dense = "Validating gene clusters...\nInconsistent T_C3\n[ True False]\n[0. 1.]\nGene Table Inconsistencies: 1\n"
    lines, count, names = model.parse_dense_stdout(dense)
    assert count == 1 and names == ['T_C3'] and lines[2] == '[ True False]'


def test_bit_packing_matches_the_library_layout():
    rng = np.random.default_rng(1)
    X = rng.random((130, 3)) < 0.5
    bits = model.pack(X)
    assert bits.shape == (3, 16) and bits.dtype == np.uint64
    assert [model.stride_words(n) for n in (0, 1, 64, 65, 1024, 1025, 150000)] == [16, 16, 16, 16, 16, 32, 2352]
    assert np.array_equal(model.unpack(bits, 130), X) and model.pad_bits_clear(bits, 130)
    assert bool((int(bits[1, 2]) >> 1) & 1) == bool(X[129, 1])
    bits[0, 2] |= np.uint64(1 << 2)
    assert not model.pad_bits_clear(bits, 130)
    for r in (0, 63, 64, 129):
        assert np.array_equal(pangenome._bitmap_row(bits, r), X[r])
