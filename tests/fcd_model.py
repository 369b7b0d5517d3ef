"""TEST INFRASTRUCTURE: a plain-numpy restatement of the greedy rule of formal concept decomposition as the device
states it (include/pgx.h, "Formal concept decomposition"; pangenomix_amd/csrc/fcd.hip), for table sizes where no
fixture of the reference exists. tests/test_fcd_host.py checks it against every fixture, so it is a fair yardstick.

    U    the ones not covered yet (starts as the table), `left` of them
    per concept: acc = the rows with a one in U, live = the columns with a one in U (ascending), cols = []
    per step:    cnt[c] = ones of U[:, c] among acc, for every live column
                 score[c] = (len(cols) + 1) * cnt[c]                                  (default)
                          = ((len(cols) + 1) ** dim_coeff) * cnt[c]   in float64      (dim_balance, not under overlap)
                          = cnt[c] + sum over acc of S[r, c] * w[r]                   (overlap; w[r] = ones of U in row r
                                                                                       among cols)
                 the best live column (np.argmax: the lowest index among equals) joins if its score is > the
                 concept's current score; acc &= U[:, c]  (S[:, c] under overlap)
    the concept is (acc ascending, cols); its block is cleared in U.
"""
import numpy as np


def decompose(S, limit=None, overlap=False, dim_balance=False, return_steps=False):
    """F in discovery order (tuples of int) of the 0/1 table S (2-D, any dtype); with return_steps also the number of
    score evaluations."""
    S = np.asarray(S) != 0
    n_rows, n_cols = S.shape
    U = S.copy()
    if limit is None:
        limit = n_rows * n_cols
    with np.errstate(divide='ignore', invalid='ignore'):
        dim_coeff = np.log(n_rows) / np.log(n_cols)
    F, steps = [], 0
    left = int(U.sum())
    while left > 0 and len(F) < limit:
        rows = np.flatnonzero(U.any(axis=1))                 # acc, as ascending row indices
        live = np.flatnonzero(U.any(axis=0)).tolist()
        Ua = U[rows]
        Sa = S[rows] if overlap else None
        w = np.zeros(rows.size, dtype=np.int64)
        cols, current = [], 0
        while rows.size and live:
            steps += 1
            cnt = Ua[:, live].sum(axis=0, dtype=np.int64)
            if overlap:
                score = cnt + (Sa[:, live] * w[:, None]).sum(axis=0, dtype=np.int64)
            elif dim_balance:
                with np.errstate(all='ignore'):
                    score = ((len(cols) + 1) ** dim_coeff) * cnt
            else:
                score = (len(cols) + 1) * cnt
            best = int(np.argmax(score))
            if not score[best] > current:
                break
            c = live.pop(best)
            cols.append(c)
            current = score[best]
            w += Ua[:, c]
            keep = (Sa if overlap else Ua)[:, c]
            rows, Ua, w = rows[keep], Ua[keep], w[keep]
            if overlap:
                Sa = Sa[keep]
        if current > 0:
            block = np.ix_(rows, cols)
            cleared = int(U[block].sum())
            if cleared == 0:
                raise RuntimeError('a concept cleared nothing')
            U[block] = False
            left -= cleared
            F.append((tuple(rows.tolist()), tuple(cols)))
    return (F, steps) if return_steps else F


def formal_concepts(S, limit=None, sort_components=True, overlap=False, dim_balance=False, seed=None):
    """F as formal_concept_decomposition returns it: decompose() around the shuffle of `seed` (numpy's global legacy
    generator, rows then columns; concepts un-shuffled into lists) and the stable sort by size, largest first."""
    S = np.asarray(S)
    if seed is None:
        F = decompose(S, limit, overlap, dim_balance)
    else:
        np.random.seed(seed)
        row_shuffle = np.arange(S.shape[0]); np.random.shuffle(row_shuffle)
        col_shuffle = np.arange(S.shape[1]); np.random.shuffle(col_shuffle)
        F = [([row_shuffle[x] for x in xs], [col_shuffle[y] for y in ys])
             for xs, ys in decompose(S[row_shuffle, :][:, col_shuffle], limit, overlap, dim_balance)]
    if sort_components:
        F = sorted(F, key=lambda f: -(len(f[0]) * len(f[1])))        # (stable: equal sizes keep their order)
    return F


def coverage(S, F):
    """compute_concept_coverage's array: the fraction of the ones of S the first i concepts cover."""
    S = np.asarray(S) != 0
    total = float(S.sum())
    uncovered, left = S.copy(), total
    out = np.zeros(len(F) + 1)
    for i, (x, y) in enumerate(F):
        block = np.ix_(np.asarray(x, dtype=np.int64), np.asarray(y, dtype=np.int64))
        left -= uncovered[block].sum()
        uncovered[block] = False
        out[i + 1] = 1.0 - left / total
    return out


def load_fixture(path):
    """A file of tests/golden/fcd (written by tests/golden/make_golden_fcd.py from a run of the reference) as a dict:
    'rows', 'cols' (int64 coordinates of the ones), 'shape', 'dtype', 'kwargs' (the reference call's keyword arguments),
    'F' (the expected concept list, with its container type), 'kind', 'key', 'pos' (generator state after the call),
    'coverage' (or None) and 'dense' (a function: the table as a dense array of the case's dtype)."""
    d = np.load(path)
    rows, cols = d['rows'].astype(np.int64), d['cols'].astype(np.int64)
    shape = tuple(int(x) for x in d['shape'])
    dtype = str(d['dtype'])
    f_rows, ro = np.cumsum(d['f_rows_delta'], dtype=np.int64), d['f_row_off']
    f_cols, co = d['f_cols'].astype(np.int64), d['f_col_off']
    kind = str(d['kind'])
    box = tuple if kind == 'tuple' else list
    F = [(box(f_rows[ro[i]:ro[i + 1]].tolist()), box(f_cols[co[i]:co[i + 1]].tolist())) for i in range(ro.size - 1)]
    kwargs = {'overlap': bool(d['overlap']), 'dim_balance': bool(d['dim_balance']),
              'sort_components': bool(d['sort_components']),
              'limit': None if int(d['limit']) < 0 else int(d['limit']), 'seed': None if int(d['seed']) < 0 else int(d['seed'])}

    def dense():
        X = np.zeros(shape, dtype=dtype)
        X[rows, cols] = 1
        return X

    return {'rows': rows, 'cols': cols, 'shape': shape, 'dtype': dtype, 'kwargs': kwargs, 'F': F, 'kind': kind,
            'key': d['key'], 'pos': int(d['pos']), 'coverage': d['coverage'] if d['coverage'].size else None, 'dense': dense}
