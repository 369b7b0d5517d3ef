"""compute_bernoulli_grid_core_genome without a GPU: LightSparseDataFrame.to_sparse_arrays() against the reference's
frame (tests/golden/core/to_sparse_arrays.npz, written by tests/golden/make_golden_core.py), and the refusals that
happen before any library call."""
import os

import numpy as np
import pandas as pd
import pytest
import scipy.sparse

from pangenomix_amd import _native, sparse_utils
from pangenomix_amd import pangenome_analysis as pa

HERE = os.path.dirname(os.path.abspath(__file__))


def lsdf_of(rows, cols, shape, index=None, columns=None, data=None):
    data = np.ones(len(rows), dtype=np.int64) if data is None else data
    m = scipy.sparse.coo_matrix((data, (rows, cols)), shape=shape)
    index = ['g%d' % i for i in range(shape[0])] if index is None else index
    columns = ['s%d' % j for j in range(shape[1])] if columns is None else columns
    return sparse_utils.LightSparseDataFrame(index, columns, m)


def test_to_sparse_arrays_equals_the_reference_frame():
    z = np.load(os.path.join(HERE, 'golden', 'core', 'to_sparse_arrays.npz'))
    frame = lsdf_of(z['rows'], z['cols'], tuple(z['shape']), list(z['index']), list(z['columns'])).to_sparse_arrays()
    assert list(frame.index) == list(z['index']) and list(frame.columns) == list(z['columns'])
    assert [str(t) for t in frame.dtypes] == list(z['dtypes'])
    for j, col in enumerate(frame.columns):
        a = frame[col].array
        assert isinstance(a, pd.arrays.SparseArray)
        assert bool(np.isnan(a.fill_value)) == bool(z['fill_is_nan'][j])
        assert a.kind == str(z['kinds'][j])
        np.testing.assert_array_equal(np.asarray(a.sp_values), z['sp_values_%d' % j])
        assert np.asarray(a.sp_values).dtype == z['sp_values_%d' % j].dtype
        np.testing.assert_array_equal(np.asarray(a.sp_index.indices), z['sp_indices_%d' % j])


@pytest.fixture
def no_library(monkeypatch):
    """Any library call fails the test: the refusals must come first."""
    def refuse(*a, **k):
        raise AssertionError('the library was called before the input was checked')
    monkeypatch.setattr(_native, 'lib', refuse)
    monkeypatch.setattr(_native, 'default_context', refuse)


@pytest.mark.parametrize('bad', [2, -1, 0.5, np.nan])
def test_dense_frame_that_is_not_binary_is_refused(no_library, bad):
    X = np.ones((5, 3))
    X[2, 1] = bad
    with pytest.raises(ValueError):
        pa.compute_bernoulli_grid_core_genome(pd.DataFrame(X, index=list('abcde'), columns=list('xyz')))


def test_lsdf_with_values_other_than_one_is_refused(no_library):
    t = lsdf_of([0, 1, 2], [0, 1, 1], (3, 2), data=np.array([1, 2, 1], dtype=np.int64))
    with pytest.raises(ValueError):
        pa.compute_bernoulli_grid_core_genome(t)


def test_lsdf_with_duplicate_coordinates_is_refused(no_library):
    t = lsdf_of([0, 1, 2, 1], [0, 1, 1, 1], (3, 2))
    with pytest.raises(ValueError):
        pa.compute_bernoulli_grid_core_genome(t)


def test_sparse_columns_with_stored_values_other_than_one_are_refused(no_library):
    frame = lsdf_of([0, 1, 2], [0, 1, 1], (3, 2), data=np.array([1, 3, 1], dtype=np.int64)).to_sparse_arrays()
    with pytest.raises(ValueError):
        pa.compute_bernoulli_grid_core_genome(frame)


def test_mixed_sparse_and_dense_columns_are_refused(no_library):
    frame = lsdf_of([0, 1, 2], [0, 1, 1], (3, 2)).to_sparse_arrays()
    frame['s1'] = np.array([0, 1, 1])
    with pytest.raises(ValueError):
        pa.compute_bernoulli_grid_core_genome(frame)


def test_there_is_no_cpu_fallback():
    """Without a usable device the call raises (PGX_ERR_NO_DEVICE); with one it runs on it."""
    try:
        _native.Context(0).close()
        have_device = True
    except _native.PgxError:
        have_device = False
    frame = pd.DataFrame(np.array([[1, 1, 0], [1, 1, 1]]), index=['a', 'b'], columns=['x', 'y', 'z'])
    if have_device:
        df_opt, res = pa.compute_bernoulli_grid_core_genome(frame)
        assert list(df_opt.columns) == ['initial', 'optimum'] and res.x.size == 5
    else:
        with pytest.raises(_native.PgxError) as err:
            pa.compute_bernoulli_grid_core_genome(frame, ctx=None)
        assert err.value.status == -2
