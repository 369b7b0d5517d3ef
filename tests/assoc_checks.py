"""TEST INFRASTRUCTURE shared by tests/test_assoc_host.py (host halves, with the numpy model standing in for the device)
and tests/test_gpu_assoc.py (the device): the comparisons of the public functions against the fixtures of
tests/golden/assoc, written once. Everything is compared exactly except the LOR (LOR_ATOL: the issue's bound -- inputs
are exact integers, a handful of roundings in numerator and denominator, one log2 of a result below 64)."""
import contextlib
import io
import warnings

import numpy as np
import pandas as pd
import scipy.sparse

import assoc_model
from pangenomix_amd import ml_pipelines, sparse_utils

LOR_ATOL = 1e-12


class ModelCtx(object):
    """Stands in for _native.Context where no device exists: the two calls the host code makes, answered by
    tests/assoc_model.py. Counts its calls."""

    def __init__(self):
        self.calls = 0

    def assoc(self, rows, genomes, n_rows, n_genomes, col_map=None, masks=None, blocks=False, drop_empty=False):
        self.calls += 1
        rows, genomes = np.asarray(rows, dtype=np.int64), np.asarray(genomes, dtype=np.int64)
        dup = rows.size - np.unique(rows * max(n_genomes, 1) + genomes).size
        if dup:
            return None, int(dup)
        X = assoc_model.dense(rows, genomes, (n_rows, n_genomes))
        if col_map is not None:
            X = X[:, np.asarray(col_map, dtype=np.int64)]
        out = {'incidence': X.sum(axis=1).astype(np.uint32), 'block_of_row': None, 'rep_row': None}
        n_targets = 0 if masks is None else len(masks)
        out['tp'] = np.zeros((n_targets, n_rows), dtype=np.uint32)
        for t in range(n_targets):
            bits = np.unpackbits(np.ascontiguousarray(masks[t]).view(np.uint8), bitorder='little')[:X.shape[1]].astype(bool)
            out['tp'][t] = (X & bits[None, :]).sum(axis=1)
        if blocks:
            if drop_empty:
                kept = np.flatnonzero(out['incidence'] > 0)
                b, rep = assoc_model.blocks(X[kept])
                out['block_of_row'] = np.full(n_rows, -1, dtype=np.int32)
                out['block_of_row'][kept] = b
                out['rep_row'] = kept[rep].astype(np.int32)
            else:
                b, rep = assoc_model.blocks(X)
                out['block_of_row'], out['rep_row'] = b.astype(np.int32), rep.astype(np.int32)
        return out, 0


def fixture_matrix(fx):
    """The fixture's table as the COO matrix the reference was given (values of the case's dtype, entries in its order)."""
    return scipy.sparse.coo_matrix((np.ones(fx['rows'].size, dtype=fx['dtype']), (fx['rows'], fx['cols'])), shape=fx['shape'])


def same_definitions(defs, block_of_row, n_blocks, types):
    want = assoc_model.definitions(block_of_row, n_blocks)
    assert type(defs).__name__ == types[0] and len(defs) == len(want)
    for got, w in zip(defs, want):
        assert type(got).__name__ == types[1] and type(got[0]).__name__ == types[2]
        assert [int(x) for x in got] == w


def check_blocks(fx, ctx, S=None):
    """compress_rows_spmatrix and compress_rows on the fixture's table (or on S, another container of the same table)."""
    coo = fixture_matrix(fx)
    n_rows, n_cols = fx['shape']
    types, n_blocks = fx['types'], fx['rep_row'].size
    spblock, defs = sparse_utils.compress_rows_spmatrix(coo if S is None else S, ctx=ctx)
    same_definitions(defs, fx['block_of_row'], n_blocks, types)
    assert spblock.format == str(fx['spblock_format']) and spblock.shape == (n_blocks, n_cols)
    spblock.sort_indices()
    assert np.array_equal(spblock.indptr, fx['spblock_indptr']) and np.array_equal(spblock.indices, fx['spblock_indices'])
    if S is None:
        assert str(spblock.dtype) == str(fx['spblock_dtype'])
    lsdf = sparse_utils.LightSparseDataFrame(['r%d' % i for i in range(n_rows)], ['c%d' % j for j in range(n_cols)], coo)
    lsdf_block, ldefs = sparse_utils.compress_rows(lsdf, ctx=ctx)
    assert isinstance(lsdf_block, sparse_utils.LightSparseDataFrame) and type(ldefs) is list
    assert lsdf_block.data.format == types[7] and lsdf_block.shape == (n_blocks, n_cols)
    assert list(lsdf_block.index) == ['B%d' % b for b in range(n_blocks)] and list(lsdf_block.columns) == list(lsdf.columns)
    assert (str(lsdf_block.index[0]), str(lsdf_block.index[-1])) == (types[5], types[6])
    assert (lsdf_block.data.tocsr() != spblock).nnz == 0
    want = assoc_model.definitions(fx['block_of_row'], n_blocks)
    for got, w in zip(ldefs, want):
        assert type(got).__name__ == types[3] and got.dtype.kind == types[4]
        assert list(got) == ['r%d' % r for r in w]


def same_lor(got, want):
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf])
    assert np.allclose(got[ok & ~inf], want[ok & ~inf], atol=LOR_ATOL, rtol=0)


def check_contingency(fx, ctx, S=None):
    """Every target of the fixture, one call each with another batch_size, then all of them in one 2-D call."""
    S = fixture_matrix(fx) if S is None else S
    targets, sizes = fx['targets'], [int(b) for b in fx['batch_sizes']]
    for k, t in enumerate(targets):
        got = ml_pipelines.contingency_tables_from_sparse(S, t, batch_size=sizes[k % len(sizes)], ctx=ctx)
        assert got.dtype == np.float64 and got.shape == fx['contingency'][k].shape
        assert np.array_equal(got, fx['contingency'][k], equal_nan=True), k
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            same_lor(ml_pipelines.adjusted_lor(got), fx['lor'][k])
    both = ml_pipelines.contingency_tables_from_sparse(S, targets, ctx=ctx)
    assert both.shape == fx['contingency'].shape and np.array_equal(both, fx['contingency'], equal_nan=True)


def prepare_inputs(d):
    """(lsdf, df_amr, df_known, drugs) of a prepare_*.npz."""
    n_rows, n_cols = (int(x) for x in d['shape'])
    rows, cols = d['rows'].astype(np.int64), d['cols'].astype(np.int64)
    index, columns = ['g%d' % i for i in range(n_rows)], ['s%d' % j for j in range(n_cols)]
    coo = scipy.sparse.coo_matrix((np.ones(rows.size, dtype=np.int64), (rows, cols)), shape=(n_rows, n_cols))
    lsdf = sparse_utils.LightSparseDataFrame(index, columns, coo)
    drugs = ['drug%d' % k for k in range(int(d['n_drugs']))]
    order = d['pheno_rows']
    df_amr = pd.DataFrame(d['pheno'][order], index=[columns[j] for j in order], columns=drugs)
    df_known = pd.DataFrame(d['known'], index=index, columns=drugs)
    return lsdf, df_amr, df_known, drugs


def check_prepare(path, ctx, lsdf=None):
    d = np.load(path)
    own, df_amr, df_known, drugs = prepare_inputs(d)
    lsdf = own if lsdf is None else lsdf
    for k, drug in enumerate(drugs):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            amr, known, feat, block, defs = ml_pipelines.prepare_amr_case_data(drug, lsdf, df_amr, df_known, ctx=ctx)
        assert buf.getvalue() == str(d['stdout_%d' % k])
        assert isinstance(amr, pd.Series) and list(amr.index) == list(d['amr_index_%d' % k])
        assert np.array_equal(amr.values, d['amr_values_%d' % k])
        assert type(known) is set and sorted(known) == list(d['known_%d' % k])
        for frame, name in ((feat, 'feat'), (block, 'block')):
            assert isinstance(frame, sparse_utils.LightSparseDataFrame) and frame.data.format == 'coo'
            assert list(frame.index) == list(d['%s_index_%d' % (name, k)])
            assert list(frame.columns) == list(d['feat_columns_%d' % k])
            assert np.array_equal(frame.data.row, d['%s_rows_%d' % (name, k)])
            assert np.array_equal(frame.data.col, d['%s_cols_%d' % (name, k)])
        off = d['def_off_%d' % k]
        assert type(defs) is list and len(defs) == off.size - 1
        for i, x in enumerate(defs):
            assert isinstance(x, np.ndarray) and list(x) == list(d['def_flat_%d' % k][off[i]:off[i + 1]])


def check_prefilter(path, ctx):
    d = np.load(path)
    n_rows, n_cols = (int(x) for x in d['shape'])
    rows, cols = d['rows'].astype(np.int64), d['cols'].astype(np.int64)
    coo = scipy.sparse.coo_matrix((np.ones(rows.size, dtype=np.int64), (rows, cols)), shape=(n_rows, n_cols))
    lsdf = sparse_utils.LightSparseDataFrame(['B%d' % i for i in range(n_rows)], ['s%d' % j for j in range(n_cols)], coo)
    y = pd.Series(d['y'], index=lsdf.columns)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        got = ml_pipelines.prefilter_features_by_lor(lsdf, y, min_freq=int(d['min_freq']), max_features=int(d['max_features']),
                                                     ctx=ctx)
    assert buf.getvalue() == str(d['stdout']) and (got is lsdf) == bool(d['same_object'])
    assert got.shape == tuple(int(x) for x in d['out_shape']) and list(got.index) == list(d['out_index'])
    assert np.array_equal(got.data.row, d['out_rows']) and np.array_equal(got.data.col, d['out_cols'])


def tie_table(rng):
    """(block x genome bool table, phenotype) built to have many equal LORs -- whole runs of rows with the same TP and
    FP, across the `half` boundary of the selections the tests ask for -- and NaN LORs for no row (a NaN needs an
    all-zero target, which the tests add separately)."""
    y = (rng.random(40) < 0.5).astype(float)
    patterns = rng.random((12, 40)) < 0.3
    X = patterns[rng.integers(0, 12, 300)]
    X[:, 0] |= ~X.any(axis=1)
    return X, y


def check_selection_against_model(X, y, min_freq, max_features, ctx):
    """prefilter_features_by_lor on its selection path against assoc_model (the reference raises there)."""
    X = np.asarray(X, dtype=bool)
    rows, cols = np.nonzero(X)
    coo = scipy.sparse.coo_matrix((np.ones(rows.size, dtype=np.int64), (rows, cols)), shape=X.shape)
    lsdf = sparse_utils.LightSparseDataFrame(['B%d' % i for i in range(X.shape[0])], ['s%d' % j for j in range(X.shape[1])], coo)
    series = pd.Series(y, index=lsdf.columns)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        got = ml_pipelines.prefilter_features_by_lor(lsdf, series, min_freq=min_freq, max_features=max_features, ctx=ctx)
    kept = np.arange(X.shape[0]) if min_freq <= 0 else np.flatnonzero(X.sum(axis=1) >= min_freq)
    assert kept.size > max_features, 'the case must reach the selection'
    lors = assoc_model.adjusted_lor(assoc_model.contingency(X[kept], y))
    want = kept[np.asarray(assoc_model.select(lors, max_features), dtype=np.int64)]
    assert list(got.index) == ['B%d' % r for r in want]
    assert np.array_equal(got.values != 0, X[want])
    assert buf.getvalue() == 'Species x drug LOR-selected compressed features: %s\n' % (got.shape,)
    return lors, want
