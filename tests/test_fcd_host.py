"""Formal concept decomposition, what can be checked without a GPU: the numpy model of the device's rule
(tests/fcd_model.py) gives the reference's F on every fixture (tests/golden/fcd, written by make_golden_fcd.py from runs
of the reference), so it is a fair yardstick where no fixture exists; the host helpers of pangenomix_amd/fcd.py behave as
the reference's; input validation; no CPU fallback."""
import glob
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import scipy.sparse

import fcd_model
from pangenomix_amd import _native, fcd, sparse_utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, 'tests', 'golden', 'fcd', '*.npz')))
NAMES = [os.path.basename(p)[:-4] for p in FIXTURES]


def same_concepts(got, want, kind):
    """equal concept lists, with the container type of every member"""
    assert len(got) == len(want)
    box = tuple if kind == 'tuple' else list
    for (gx, gy), (wx, wy) in zip(got, want):
        assert type(gx) is box and type(gy) is box
        assert list(gx) == list(wx) and list(gy) == list(wy)


def test_the_fixture_set_is_complete():
    assert len(FIXTURES) >= 22
    for must in ('pancore_12000x100_limit400', 'all_zeros', 'all_ones', 'one_row', 'one_column', 'limit_0', 'rows_193',
                 'duplicate_rows', 'bool_input', 'float_input'):
        assert must in NAMES
    largest_older = max(os.path.getsize(p) for p in glob.glob(os.path.join(ROOT, 'tests', 'golden', '*', '*.npz'))
                        if os.sep + 'fcd' + os.sep not in p)
    assert max(os.path.getsize(p) for p in FIXTURES) <= largest_older


@pytest.mark.parametrize('path', FIXTURES, ids=NAMES)
def test_model_equals_the_reference_on_every_fixture(path):
    fx = fcd_model.load_fixture(path)
    np.random.seed(12345)
    got = fcd_model.formal_concepts(fx['dense'](), **fx['kwargs'])
    same_concepts(got, fx['F'], fx['kind'])
    st = np.random.get_state()
    assert st[2] == fx['pos'] and np.array_equal(st[1], fx['key'])
    if fx['coverage'] is not None:
        assert np.array_equal(fcd_model.coverage(fx['dense'](), fx['F']), fx['coverage'])


def test_pancore_fixture_is_the_synthetic_table_and_is_covered():
    from pangenomix_amd import synth
    fx = fcd_model.load_fixture(os.path.join(ROOT, 'tests', 'golden', 'fcd', 'pancore_12000x100_limit400.npz'))
    r, c, G = synth.pancore_matrix(12000, 100, 1)
    order = np.lexsort((c, r))
    assert fx['shape'] == (G, 100) and np.array_equal(fx['rows'], r[order]) and np.array_equal(fx['cols'], c[order])
    assert len(fx['F']) == 111
    assert sum(len(x) * len(y) for x, y in fx['F']) == r.size         # no overlap: every one is covered exactly once


def test_fcd_is_reachable_from_the_package_and_imports_without_seaborn():
    import pangenomix_amd
    assert pangenomix_amd.fcd is fcd
    code = ('import sys\nsys.modules["seaborn"] = None\nimport pangenomix_amd.fcd as f\n'
            'assert "seaborn" not in [m for m in sys.modules if sys.modules[m] is not None]\nprint(f.__name__)')
    out = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == 'pangenomix_amd.fcd', out.stderr


def test_signature_mirrors_the_reference():
    import inspect
    sig = inspect.signature(fcd.formal_concept_decomposition)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [
        ('S', inspect.Parameter.empty), ('limit', None), ('sort_components', True), ('overlap', False),
        ('dim_balance', False), ('seed', None), ('verbose', False), ('ctx', None)]
    sig = inspect.signature(fcd.compute_concept_coverage)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [
        ('S', inspect.Parameter.empty), ('F', inspect.Parameter.empty), ('plot', False), ('log_rate', 50), ('ctx', None)]


F3 = [((0, 2), (1,)), ((1, 2, 3), (0, 2)), ((3,), (3, 1))]


def test_decompose_and_encode():
    S = np.zeros((4, 4), dtype=np.int64)
    W, H = fcd.decompose_from_concepts(S, F3)
    assert W.dtype == np.dtype(int) and H.dtype == np.dtype(int) and W.shape == (4, 3) and H.shape == (3, 4)
    assert W.T.tolist() == [[1, 0, 1, 0], [0, 1, 1, 1], [0, 0, 0, 1]]
    assert H.tolist() == [[0, 1, 0, 0], [1, 0, 1, 0], [0, 1, 0, 1]]
    assert np.array_equal(fcd.encode_from_concepts(F3), H)
    assert fcd.encode_from_concepts(F3[:2]).shape == (2, 3)            # as wide as the largest column index needs
    W0, H0 = fcd.decompose_from_concepts(S, [])
    assert W0.shape == (4, 0) and H0.shape == (0, 4)
    Wl, Hl = fcd.decompose_from_concepts(S, [([np.int64(0), np.int64(2)], [np.int64(1)])])    # a seeded run's lists
    assert np.array_equal(Wl[:, 0], W[:, 0]) and np.array_equal(Hl[0], H[0])


def test_sort_is_stable_and_largest_first():
    F = [((0,), (0,)), ((0, 1), (0, 1)), ((5,), (7,)), ((1, 2, 3), (0, 1)), ((9, 8), (1, 2))]
    assert fcd.sort_concepts_by_size(F) == [F[3], F[1], F[4], F[0], F[2]]


def test_save_load_round_trip_and_file_bytes(tmp_path):
    path = str(tmp_path / 'concepts.txt')
    fcd.save_formal_concepts(F3, path)
    assert open(path, 'rb').read() == b'0|0,2|1\n1|1,2,3|0,2\n2|3|3,1'
    assert fcd.load_formal_concepts(path) == F3
    assert fcd.load_formal_concepts(path, sort_components=True) == [F3[1], F3[0], F3[2]]
    fcd.save_formal_concepts([([np.int64(4), np.int64(1)], [np.int64(0)])], path)
    assert open(path, 'rb').read() == b'0|4,1|0'


def test_save_full_writes_labelled_matrices(tmp_path):
    table = pd.DataFrame(np.zeros((4, 4), dtype=int), index=['a', 'b', 'c', 'd'], columns=['w', 'x', 'y', 'z'])
    pw, ph, pf = (str(tmp_path / n) for n in ('W.csv', 'H.csv', 'F.txt'))
    fcd.save_formal_concepts_full(F3, pw, ph, pf, table)
    assert open(pw).read() == ',FCD_0,FCD_1,FCD_2\na,1.0,,\nb,,1.0,\nc,1.0,1.0,\nd,,1.0,1.0\n'
    assert open(ph).read() == ',w,x,y,z\nFCD_0,,1.0,,\nFCD_1,1.0,,1.0,\nFCD_2,,1.0,,1.0\n'
    assert fcd.load_formal_concepts(pf) == F3


def test_similarity_score():
    S = np.ones((4, 4), dtype=int)
    assert fcd.compute_concept_list_similarity(F3, F3, S) == (2 + 6 + 2) / 16.0
    # greedy in the order of F1: its first concept takes the best partner (the first among equals) and keeps it
    F2 = [((0, 2, 3), (1, 3)), ((0, 2), (1,))]
    assert fcd.compute_concept_list_similarity(F3, F2, S) == (2 + 0) / 16.0
    assert fcd.compute_concept_list_similarity([], F3, S) == 0.0


@pytest.mark.parametrize('bad', [np.array([[0, 2], [1, 0]]), np.array([[0.5, 1.0]]), np.array([[np.nan, 1.0]]),
                                 np.array([[-1, 1]]), np.array([0, 1, 1])])
def test_tables_that_are_not_binary_are_refused_before_any_device_call(bad):
    with pytest.raises(ValueError):
        fcd.formal_concept_decomposition(bad)
    if bad.ndim == 2:
        with pytest.raises(ValueError):
            fcd.formal_concept_decomposition(scipy.sparse.coo_matrix(bad))
        with pytest.raises(ValueError):
            fcd.compute_concept_coverage(bad, [])


def test_inputs_are_read_through_their_coordinates():
    X = np.array([[1, 0, 1], [0, 0, 1]])
    want = ([0, 0, 1], [0, 2, 2], (2, 3))
    for S in (X, X.astype(bool), X.astype(float), scipy.sparse.csr_matrix(X), scipy.sparse.coo_matrix(X),
              sparse_utils.LightSparseDataFrame(['a', 'b'], ['x', 'y', 'z'], scipy.sparse.coo_matrix(X))):
        rows, cols, shape, resident = fcd._table(S)
        assert (rows.tolist(), cols.tolist(), tuple(shape)) == want and resident is None
    stored_zero = scipy.sparse.coo_matrix(([1, 0, 1, 1], ([0, 1, 0, 1], [0, 0, 2, 2])), shape=(2, 3))
    assert fcd._table(stored_zero)[0].tolist() == [0, 0, 1]


def test_dim_balance_factors_are_the_reference_expression():
    got = fcd._dim_factors(12000, 100)
    dim_coeff = np.log(12000) / np.log(100)
    assert got.dtype == np.float64 and got.shape == (100,)
    assert all(got[k] == (k + 1) ** dim_coeff for k in range(100))
    with np.errstate(all='ignore'):
        assert fcd._dim_factors(200, 1).tolist() == [1.0]            # 1 ** inf


def test_no_cpu_fallback_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip('a GPU is present')
    with pytest.raises(_native.PgxError, match='no usable HIP device|no CPU fallback'):
        fcd.formal_concept_decomposition(np.array([[1, 0], [1, 1]]))
    with pytest.raises(_native.PgxError, match='no usable HIP device|no CPU fallback'):
        fcd.compute_concept_coverage(np.array([[1, 0], [1, 1]]), [((0, 1), (0,))])
