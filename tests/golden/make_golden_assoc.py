#!/usr/bin/env python
"""Golden fixtures for the association screen (reference sparse_utils.py compress_rows / compress_rows_spmatrix and
ml_pipelines.py contingency_tables_from_sparse / adjusted_lor / prefilter_features_by_lor / prepare_amr_case_data),
produced by RUNNING THE REFERENCE in the build container (needs /root/reference; it never travels to the GPU box):

    python tests/golden/make_golden_assoc.py

The reference's ml_pipelines imports `amr_pangenome.sparse_utils`, a package the reference does not ship: that name is
registered in sys.modules pointing at the reference's own pangenomix.sparse_utils before the import. Nothing of sklearn
is called. Only data is written: coordinates, targets, returned arrays, container types as strings.

tests/golden/assoc/table_<case>.npz
  rows, cols, shape, dtype   the table's stored entries as COO coordinates IN THE ORDER they were handed over, and the
                             dtype of its values (all 1)
  block_of_row, rep_row      compress_rows_spmatrix: the block of every row (from the returned definitions) and the first
                             row of every block; spblock_indptr / spblock_indices / spblock_format / spblock_dtype: the
                             returned matrix
  types                      type names: the definitions' container, a definition, its elements (compress_rows_spmatrix),
                             then a definition and the kind of its dtype, the block labels' first and last, and the
                             format of the block LSDF's matrix (compress_rows on an LSDF labelled r0.. / c0..)
  targets [K, n_samples], contingency [K, n_rows, 4], lor [K, n_rows]     contingency_tables_from_sparse + adjusted_lor
                             for every target (all-zero, all-one, 0/1, with NaN, non-binary floats); batch_sizes: the
                             batch sizes tried (below, at and above the row count): the generator asserts that the
                             reference's result is the same for all of them
tests/golden/assoc/prepare_<case>.npz    prepare_amr_case_data: table as above with labels g<i> / s<j>, the phenotype
  frame `pheno` [n_genomes, n_drugs] (NaN = no phenotype) in the row order `pheno_rows` (a permutation of the genomes: the
  frame need not be in the table's order), `known` [n_rows, n_drugs]; per drug d: amr_index_d, amr_values_d, known_d,
  feat_index_d, feat_rows_d, feat_cols_d, block_rows_d, block_cols_d, def_flat_d, def_off_d, stdout_d
tests/golden/assoc/prefilter_<case>.npz  prefilter_features_by_lor on the paths the reference can run: block table, phenotype,
  min_freq, max_features, the returned index labels and coordinates

Cases on which the reference raises are recorded here and dropped, not given an invented expectation:
  prefilter_features_by_lor with more rows than max_features after the frequency filter: TypeError (slice indices must be
  integers: `max_features/2` is a float under Python 3). The selection behind it is defined in DESIGN.md 6d and checked
  against tests/assoc_model.py.
"""
import contextlib
import io
import os
import sys
import warnings

import numpy as np
import pandas as pd
import scipy.sparse

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, '/root/reference')

import pangenomix.sparse_utils as ref_su      # noqa: E402
import types                                   # noqa: E402
_pkg = types.ModuleType('amr_pangenome')
_pkg.sparse_utils = ref_su
sys.modules.setdefault('amr_pangenome', _pkg)
sys.modules.setdefault('amr_pangenome.sparse_utils', ref_su)
import pangenomix.ml_pipelines as ref_ml      # noqa: E402

OUT = os.path.join(HERE, 'assoc')


def random_table(rng, n_rows, n_cols, n_patterns=None, empty=(), density=0.15):
    """bool table; with n_patterns the rows are drawn from that many patterns (many duplicate rows)."""
    if n_patterns is None:
        X = rng.random((n_rows, n_cols)) < rng.beta(0.5, 2.0, n_rows)[:, None] * 2 * density * 3
    else:
        P = rng.random((n_patterns, n_cols)) < density
        X = P[rng.integers(0, n_patterns, n_rows)]
    X = np.array(X)
    for r in empty:
        X[r] = False
    return X


def targets_for(rng, n):
    t = np.zeros((6, n))
    t[1] = 1.0
    t[2] = rng.random(n) < 0.4
    t[3] = rng.random(n) < 0.6
    t[3, rng.random(n) < 0.2] = np.nan
    t[4] = np.round(rng.random(n) * 3, 2) * (rng.random(n) < 0.7)       # non-binary floats, some zero
    t[5] = rng.random(n) < 0.05
    return t


def table_case(name, X, rng, dtype='int64', scramble=False):
    X = np.asarray(X, dtype=bool)
    n_rows, n_cols = X.shape
    rows, cols = np.nonzero(X)
    if scramble:
        p = rng.permutation(rows.size)
        rows, cols = rows[p], cols[p]
    coo = scipy.sparse.coo_matrix((np.ones(rows.size, dtype=dtype), (rows, cols)), shape=X.shape)
    spblock, defs = ref_su.compress_rows_spmatrix(coo)
    block_of_row = np.full(n_rows, -1, dtype=np.int32)
    for b, members in enumerate(defs):
        assert list(members) == sorted(members)
        block_of_row[np.asarray(members, dtype=np.int64)] = b
    rep_row = np.array([m[0] for m in defs], dtype=np.int32)
    lsdf = ref_su.LightSparseDataFrame(['r%d' % i for i in range(n_rows)], ['c%d' % j for j in range(n_cols)], coo)
    lsdf_block, ldefs = ref_su.compress_rows(lsdf)
    assert all(list(a) == ['r%d' % i for i in d] for a, d in zip(ldefs, defs))
    assert (lsdf_block.data.tocsr() != spblock).nnz == 0
    tn = lambda x: type(x).__name__                                      # noqa: E731
    typ = [tn(defs), tn(defs[0]) if defs else '', tn(defs[0][0]) if defs else '',
           tn(ldefs[0]) if ldefs else '', ldefs[0].dtype.kind if ldefs else '',
           str(lsdf_block.index[0]) if defs else '', str(lsdf_block.index[-1]) if defs else '', lsdf_block.data.format]
    targets = targets_for(rng, n_cols)
    batch_sizes = sorted({max(1, n_rows // 3), max(1, n_rows), n_rows + 7, 10000})
    cont = np.zeros((targets.shape[0], n_rows, 4))
    lor = np.zeros((targets.shape[0], n_rows))
    for k, t in enumerate(targets):
        got = [ref_ml.contingency_tables_from_sparse(coo, t, batch_size=b) for b in batch_sizes]
        for g in got[1:]:
            assert np.array_equal(g, got[0], equal_nan=True), (name, k)
        cont[k] = got[0]
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            lor[k] = ref_ml.adjusted_lor(got[0])
    path = os.path.join(OUT, 'table_%s.npz' % name)
    narrow = lambda a, n: a.astype(np.uint8 if n <= 256 else np.uint16 if n <= 65536 else np.uint32)   # noqa: E731
    np.savez_compressed(path, rows=narrow(rows, n_rows), cols=narrow(cols, n_cols), shape=np.array(X.shape, dtype=np.int64),
                        dtype=np.array(dtype), block_of_row=block_of_row, rep_row=rep_row,
                        spblock_indptr=spblock.indptr, spblock_indices=spblock.indices, spblock_format=np.array(spblock.format),
                        spblock_dtype=np.array(str(spblock.dtype)), types=np.array(typ), targets=targets,
                        batch_sizes=np.array(batch_sizes), contingency=cont, lor=lor)
    print('%s: %s, %d ones, %d blocks, %d bytes' % (name, X.shape, rows.size, len(defs), os.path.getsize(path)))


def prepare_case(name, X, rng, n_drugs=3):
    X = np.asarray(X, dtype=bool)
    n_rows, n_cols = X.shape
    rows, cols = np.nonzero(X)
    index = ['g%d' % i for i in range(n_rows)]
    columns = ['s%d' % j for j in range(n_cols)]
    coo = scipy.sparse.coo_matrix((np.ones(rows.size, dtype=np.int64), (rows, cols)), shape=X.shape)
    lsdf = ref_su.LightSparseDataFrame(index, columns, coo)
    pheno = (rng.random((n_cols, n_drugs)) < 0.4).astype(float)
    pheno[rng.random((n_cols, n_drugs)) < 0.35] = np.nan
    pheno_rows = rng.permutation(n_cols)
    drugs = ['drug%d' % d for d in range(n_drugs)]
    df_amr = pd.DataFrame(pheno[pheno_rows], index=[columns[j] for j in pheno_rows], columns=drugs)
    known = np.where(rng.random((n_rows, n_drugs)) < 0.05, 1.0, np.nan)
    df_known = pd.DataFrame(known, index=index, columns=drugs)
    out = {'rows': rows.astype(np.uint16), 'cols': cols.astype(np.uint16), 'shape': np.array(X.shape, dtype=np.int64),
           'pheno': pheno, 'pheno_rows': pheno_rows, 'known': known, 'n_drugs': np.int64(n_drugs)}
    for d, drug in enumerate(drugs):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            amr, known_set, feat, block, defs = ref_ml.prepare_amr_case_data(drug, lsdf, df_amr, df_known)
        assert isinstance(amr, pd.Series) and isinstance(known_set, set) and isinstance(defs, list)
        off = np.zeros(len(defs) + 1, dtype=np.int64)
        for i, x in enumerate(defs):
            assert isinstance(x, np.ndarray)
            off[i + 1] = off[i] + len(x)
        out.update({'amr_index_%d' % d: np.array(amr.index.tolist()), 'amr_values_%d' % d: amr.values,
                    'known_%d' % d: np.array(sorted(known_set)), 'feat_index_%d' % d: np.array(feat.index.tolist()),
                    'feat_columns_%d' % d: np.array(feat.columns.tolist()),
                    'feat_rows_%d' % d: feat.data.row, 'feat_cols_%d' % d: feat.data.col,
                    'block_index_%d' % d: np.array(block.index.tolist()),
                    'block_rows_%d' % d: block.data.row, 'block_cols_%d' % d: block.data.col,
                    'def_flat_%d' % d: np.array([v for x in defs for v in x]), 'def_off_%d' % d: off,
                    'stdout_%d' % d: np.array(buf.getvalue())})
    path = os.path.join(OUT, 'prepare_%s.npz' % name)
    np.savez_compressed(path, **out)
    print('%s: %s, %d bytes' % (name, X.shape, os.path.getsize(path)))


def prefilter_case(name, X, rng, min_freq, max_features):
    X = np.asarray(X, dtype=bool)
    n_rows, n_cols = X.shape
    rows, cols = np.nonzero(X)
    coo = scipy.sparse.coo_matrix((np.ones(rows.size, dtype=np.int64), (rows, cols)), shape=X.shape)
    lsdf = ref_su.LightSparseDataFrame(['B%d' % i for i in range(n_rows)], ['s%d' % j for j in range(n_cols)], coo)
    y = pd.Series((rng.random(n_cols) < 0.4).astype(float), index=lsdf.columns)
    try:
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            got = ref_ml.prefilter_features_by_lor(lsdf, y, min_freq=min_freq, max_features=max_features)
    except Exception as e:                   # noqa: BLE001 (recorded in the docstring above, case dropped)
        print('%s: the reference raised %s: %s -- dropped' % (name, type(e).__name__, e))
        return
    path = os.path.join(OUT, 'prefilter_%s.npz' % name)
    np.savez_compressed(path, rows=rows.astype(np.uint16), cols=cols.astype(np.uint16), shape=np.array(X.shape, dtype=np.int64),
                        y=y.values, min_freq=np.int64(min_freq), max_features=np.int64(max_features),
                        out_index=np.array(got.index.tolist()), out_rows=got.data.row, out_cols=got.data.col,
                        out_shape=np.array(got.shape, dtype=np.int64), same_object=np.bool_(got is lsdf),
                        stdout=np.array(buf.getvalue()))
    print('%s: %s -> %s, %d bytes' % (name, X.shape, got.shape, os.path.getsize(path)))


def main():
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(33)
    table_case('one_sample', random_table(rng, 130, 1, density=0.5), rng)
    table_case('samples_63', random_table(rng, 193, 63, n_patterns=40), rng)
    table_case('samples_64', random_table(rng, 257, 64, n_patterns=300, empty=(0, 1)), rng)
    table_case('samples_65_empty_last', random_table(rng, 200, 65, n_patterns=25, empty=(17, 199)), rng)
    table_case('samples_400', random_table(rng, 1200, 400, empty=(0, 700, 1199)), rng)
    table_case('samples_400_duplicates', random_table(rng, 3001, 400, n_patterns=90, density=0.3), rng)
    table_case('samples_1000_scrambled', random_table(rng, 333, 1000, n_patterns=150, density=0.05), rng, scramble=True)
    table_case('no_duplicates', np.array([[(i >> b) & 1 for b in range(9)] for i in range(1, 321)], dtype=bool), rng)
    table_case('all_equal', np.tile(rng.random(70) < 0.5, (129, 1)), rng)
    table_case('all_empty', np.zeros((65, 12), dtype=bool), rng)
    table_case('float_values', random_table(rng, 100, 30, n_patterns=20), rng, dtype='float64')
    table_case('bool_values_scrambled', random_table(rng, 100, 70, n_patterns=20), rng, dtype='bool', scramble=True)
    # rows 3 and 4 differ only in a genome without a phenotype for drug0/1/2 at times: equal only after the selection
    P = random_table(rng, 260, 90, n_patterns=60, density=0.2, empty=(5,))
    P[4] = P[3]
    P[4, 11] = ~P[3, 11]
    prepare_case('260x90', P, rng)
    prepare_case('90x130_sparse', random_table(rng, 90, 130, density=0.02), rng)
    B = random_table(rng, 400, 80, density=0.2)
    prefilter_case('min_freq_0_all_kept', B, rng, 0, 400)
    prefilter_case('min_freq_3_below_max', B, rng, 3, 10000)
    prefilter_case('min_freq_30_below_max', B, rng, 30, 400)
    prefilter_case('selection_raises', B, rng, 0, 100)


if __name__ == '__main__':
    main()
