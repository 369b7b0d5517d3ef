#!/usr/bin/env python
"""Golden fixtures for formal_concept_decomposition and compute_concept_coverage (reference fcd.py), produced by RUNNING
THE REFERENCE in the build container (needs /root/reference; it never travels to the GPU box):

    python tests/golden/make_golden_fcd.py

The reference module imports seaborn at module level (for a plot call that no longer exists in seaborn); seaborn is not
installed, so an empty placeholder module of that name is registered first. Nothing of it is called.

For every case, tests/golden/fcd/<case>.npz holds
  rows, cols, shape     the table's ones as COO coordinates (row-major order, the smallest unsigned dtype that holds
                        them: sorted and narrow, the deflated file stays within the size of the largest older fixture)
                        and its shape
  dtype                 the dtype of the dense array handed to the reference ('int64', 'bool', 'float64')
  limit, seed           the arguments (-1 = None); overlap, dim_balance, sort_components as given
  f_rows_delta, f_row_off, f_cols, f_col_off     the returned F: the concepts' rows / columns end to end and n + 1
                        offsets; the rows as first differences (f_rows = cumsum(f_rows_delta): runs of neighbouring rows
                        deflate to a fraction of the indices themselves). tests/fcd_model.py:load_fixture reads a file.
  kind                  'tuple' or 'list': the container type of every concept's two members
  key, pos              the legacy generator's state after the call (seeded cases; else the state before = after)
  coverage              compute_concept_coverage(S, F) of the reference (two cases; else empty)
W and H are not stored: they follow from F and the shape (decompose_from_concepts), and the tests check W @ H against S.

Cases the reference itself fails on are recorded here and dropped, not given an invented expectation:
  (none: the bool, the float and the one-column table all run; one column makes the reference divide by log(1) = 0,
   which numpy answers with a warning and an inf that no step uses)
Not a fixture on purpose: `seed` together with `overlap`. There the reference takes the overlap terms and the row update
from the table as it was BEFORE the shuffle while the row and column numbers are those after it, so what it returns are
not all-ones blocks of S. pangenomix_amd reads the shuffled table throughout; tests/test_gpu_fcd.py checks
that combination against tests/fcd_model.py and (W @ H > 0) == S.
"""
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, '/root/reference')
sys.modules.setdefault('seaborn', types.ModuleType('seaborn'))

import pangenomix.fcd as ref_fcd              # noqa: E402
from pangenomix_amd import synth              # noqa: E402

OUT = os.path.join(HERE, 'fcd')


def blocks_table(rng, n_rows, n_cols, n_blocks, noise):
    """A table of overlapping random blocks plus a little noise: concepts of many sizes."""
    X = np.zeros((n_rows, n_cols), dtype=bool)
    for _ in range(n_blocks):
        r = rng.choice(n_rows, size=int(rng.integers(1, max(2, n_rows // 3))), replace=False)
        c = rng.choice(n_cols, size=int(rng.integers(1, max(2, n_cols // 3))), replace=False)
        X[np.ix_(r, c)] = True
    X |= rng.random((n_rows, n_cols)) < noise
    return X


def case(name, X, dtype='int64', with_coverage=False, **kwargs):
    S = np.asarray(X).astype(dtype)
    np.random.seed(12345)                       # a known state: unseeded calls must leave it alone
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        try:
            W, H, F = ref_fcd.formal_concept_decomposition(S, **kwargs)
        except Exception as e:                   # noqa: BLE001 (recorded in the docstring above, case dropped)
            print('%s: the reference raised %s: %s -- dropped' % (name, type(e).__name__, e))
            return
    st = np.random.get_state()
    kinds = {type(part).__name__ for concept in F for part in concept}
    assert len(kinds) <= 1 and all(type(concept) is tuple for concept in F), kinds
    kind = kinds.pop() if kinds else ('tuple' if kwargs.get('seed') is None else 'list')
    ro, co = np.zeros(len(F) + 1, dtype=np.int64), np.zeros(len(F) + 1, dtype=np.int64)
    for i, (x, y) in enumerate(F):
        ro[i + 1], co[i + 1] = ro[i] + len(x), co[i] + len(y)
    f_rows = np.array([v for x, _ in F for v in x], dtype=np.int32)
    f_cols = np.array([v for _, y in F for v in y], dtype=np.int32)
    cov = np.zeros(0)
    if with_coverage:
        cov = ref_fcd.compute_concept_coverage(S, F, log_rate=0)
    rows, cols = np.nonzero(np.asarray(X) != 0)
    narrow = lambda a, n: a.astype(np.uint8 if n <= 256 else np.uint16 if n <= 65536 else np.uint32)   # noqa: E731
    limit, seed = kwargs.get('limit'), kwargs.get('seed')
    np.savez_compressed(os.path.join(OUT, name + '.npz'), rows=narrow(rows, S.shape[0]), cols=narrow(cols, S.shape[1]),
                        shape=np.array(S.shape, dtype=np.int64), dtype=np.array(dtype),
                        limit=np.int64(-1 if limit is None else limit), seed=np.int64(-1 if seed is None else seed),
                        overlap=np.bool_(kwargs.get('overlap', False)), dim_balance=np.bool_(kwargs.get('dim_balance', False)),
                        sort_components=np.bool_(kwargs.get('sort_components', True)),
                        f_rows_delta=np.diff(f_rows, prepend=np.int32(0)).astype(np.int32), f_row_off=ro,
                        f_cols=f_cols, f_col_off=co, kind=np.array(kind), key=st[1], pos=np.int64(st[2]), coverage=cov)
    print('%s: %s %s, %d ones, %d concepts (%s), %d bytes' % (name, S.shape, dtype, rows.size, len(F), kind,
                                                              os.path.getsize(os.path.join(OUT, name + '.npz'))))


def main():
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(21)
    A = blocks_table(rng, 3000, 120, 14, 0.004)
    case('blocks_3000x120', A, with_coverage=True)
    case('blocks_3000x120_unsorted', A, sort_components=False)
    case('blocks_3000x120_dim_balance', A, dim_balance=True)
    case('blocks_3000x120_limit', A, limit=17)
    case('blocks_3000x120_seed', A, seed=7)
    B = blocks_table(rng, 1500, 90, 16, 0.01)
    case('blocks_1500x90_overlap', B, overlap=True, with_coverage=True)
    case('blocks_1500x90_overlap_dim_balance', B, overlap=True, dim_balance=True, sort_components=False)
    case('blocks_1500x90_seed_limit', B, seed=3, limit=25)
    case('blocks_1500x90_seed_dim_balance', B, seed=11, dim_balance=True, sort_components=False)
    C = blocks_table(rng, 333, 1000, 20, 0.003)              # more columns than rows: dim_coeff < 1
    case('wide_333x1000_dim_balance', C, dim_balance=True)
    r, c, G = synth.pancore_matrix(12000, 100, 1)
    P = np.zeros((G, 100), dtype=bool)
    P[r, c] = True
    case('pancore_12000x100_limit400', P, limit=400)
    # edge cases
    case('all_zeros', np.zeros((70, 9), dtype=bool))
    case('all_ones', np.ones((130, 11), dtype=bool))
    case('one_row', rng.random((1, 40)) < 0.5)
    case('one_column', rng.random((200, 1)) < 0.5)
    case('one_column_dim_balance', rng.random((200, 1)) < 0.5, dim_balance=True)
    case('limit_0', A[:100, :20], limit=0)
    D = blocks_table(rng, 193, 17, 9, 0.03)                  # rows not a multiple of 64
    case('rows_193', D)
    case('rows_193_seed', D, seed=1)
    case('duplicate_rows', np.repeat(blocks_table(rng, 40, 13, 6, 0.05), 5, axis=0))
    case('bool_input', D, dtype='bool', overlap=True)
    case('float_input', D, dtype='float64', dim_balance=True)


if __name__ == '__main__':
    main()
