"""TEST INFRASTRUCTURE: a numpy restatement of the rule of compute_concept_list_similarity (reference fcd.py:168-196) as
the device states it (include/pgx.h, "Comparing two concept lists"), and the cases the similarity tests share.

    A[i, r] = 1 when concept i lists row r, B[i, c] likewise for columns (a set: listed twice counts once)
    O = (A1 @ A2.T) * (B1 @ B2.T)                       the cells two concepts share
    for i = 0 .. min(n1, n2): j = argmax of O[i] over the unmatched j (np.argmax: the first among equals), j retires

tests/test_fcd_similarity_host.py checks it against the reference's recorded scores and the host loop on every case.
"""
import functools
import os

import numpy as np
import scipy.sparse

import fcd_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'fcd')
SCORES = os.path.join(ROOT, 'tests', 'golden', 'fcd_similarity', 'scores.json')


def indicator(parts, n):
    """parts: one index list per concept -> float32 0/1 matrix len(parts) x n (sums below 2^24 are exact in float32)"""
    assert n < 2 ** 24
    M = np.zeros((len(parts), max(n, 1)), dtype=np.float32)
    for i, p in enumerate(parts):
        M[i, np.asarray(p, dtype=np.int64)] = 1.0
    return M


def overlaps(F1, F2, shape):
    """O, int64, len(F1) x len(F2)"""
    n_rows, n_cols = shape
    rows = indicator([f[0] for f in F1], n_rows) @ indicator([f[0] for f in F2], n_rows).T
    cols = indicator([f[1] for f in F1], n_cols) @ indicator([f[1] for f in F2], n_cols).T
    return rows.astype(np.int64) * cols.astype(np.int64)


def pairing(O):
    """(match int64[k], overlap int64[k], total int) of the greedy rule on the overlap matrix O"""
    n1, n2 = O.shape
    k = min(n1, n2)
    free = np.ones(n2, dtype=bool)
    match, overlap = np.zeros(k, dtype=np.int64), np.zeros(k, dtype=np.int64)
    for i in range(k):
        j = int(np.argmax(np.where(free, O[i], -1)))
        free[j] = False
        match[i], overlap[i] = j, O[i, j]
    return match, overlap, int(overlap.sum())


def pack(parts, n, stride):
    """concept-major bit masks, uint64 [len(parts), stride]: bit r & 63 of word r >> 6 = index r; pad bits zero"""
    bits = np.zeros((len(parts), stride * 64), dtype=bool)
    for i, p in enumerate(parts):
        bits[i, np.asarray(p, dtype=np.int64)] = True
    assert not bits[:, n:].any()
    return np.packbits(bits, axis=1, bitorder='little').view('<u8').astype(np.uint64).reshape(len(parts), stride)


# ---- the cases ----------------------------------------------------------------------------------------------------------
GROUPS = (('blocks_3000x120', 'blocks_3000x120_unsorted', 'blocks_3000x120_limit', 'blocks_3000x120_seed',
           'blocks_3000x120_dim_balance'),
          ('blocks_1500x90_overlap', 'blocks_1500x90_seed_limit', 'blocks_1500x90_seed_dim_balance',
           'blocks_1500x90_overlap_dim_balance'),
          ('rows_193', 'rows_193_seed'))
SELF = ('pancore_12000x100_limit400', 'wide_333x1000_dim_balance', 'duplicate_rows', 'all_ones', 'one_row', 'one_column',
        'limit_0', 'all_zeros')
FIXTURE_PAIRS = [(a, b) for group in GROUPS for a in group for b in group if a != b or a == group[0]] + [(a, a) for a in SELF]
assert len(FIXTURE_PAIRS) == 45

# (n_rows, n_cols), (n1, n2), disjoint rows
GENERATED = [((1, 1), (1, 1), False), ((1, 1), (3, 70), False), ((63, 65), (70, 3), False), ((64, 1), (3, 70), False),
             ((65, 400), (257, 130), False), ((1025, 3), (70, 3), False), ((1025, 3), (257, 130), False),
             ((70001, 65), (3, 70), False), ((70001, 65), (70, 3), True), ((70001, 65), (257, 130), False),
             ((150000, 400), (1, 1), False), ((150000, 400), (257, 130), False)]


def generated_name(shape, counts, disjoint):
    return 'gen_%dx%d_%dx%d%s' % (shape + counts + ('_disjoint' if disjoint else '',))


CASES = ['%s__%s' % p for p in FIXTURE_PAIRS] + [generated_name(*g) for g in GENERATED]


def family(rng, n_rows, n_cols, n, row_lo, row_hi):
    """n concepts as (list of rows, list of columns), not a decomposition: indices drawn with replacement from
    [row_lo, row_hi) and [0, n_cols) (so some repeat); then, as far as n allows: concept 0 lists its first row and its
    first column twice, concept 1 has no rows, concept 2 no columns, concept 4 is concept 3 again. Of a range of more
    than 2048 rows only the first, the middle and the last 300 are drawn from: the concepts stay small enough for the
    host loop's sets and still share rows, in the first and in the last mask words."""
    pool = np.arange(row_lo, row_hi)
    if pool.size > 2048:
        mid = pool.size // 2
        pool = np.concatenate((pool[:300], pool[mid:mid + 300], pool[-300:]))
    F = []
    for _ in range(n):
        x = pool[rng.integers(0, pool.size, size=int(rng.integers(1, min(pool.size, 200) + 1)))].tolist()
        y = rng.integers(0, n_cols, size=int(rng.integers(1, min(n_cols, 40) + 1))).tolist()
        F.append((x, y))
    F[0] = (F[0][0] + F[0][0][:1], F[0][1] + F[0][1][:1])
    if n >= 3:
        F[1] = ([], F[1][1])
        F[2] = (F[2][0], [])
    if n >= 5:
        F[4] = (list(F[3][0]), list(F[3][1]))
    return F


@functools.lru_cache(maxsize=None)
def fixture(name):
    return fcd_model.load_fixture(os.path.join(GOLDEN, name + '.npz'))


def case_inputs(name):
    """(F1, F2, S): the two concept lists and the table of a case. Fixture pairs: the first fixture's dense table.
    Generated lists: a sparse table of the case's shape with a one in every row of its first column, up to 7."""
    if not name.startswith('gen_'):
        a, b = name.split('__')
        return fixture(a)['F'], fixture(b)['F'], fixture(a)['dense']()
    for i, (shape, counts, disjoint) in enumerate(GENERATED):
        if generated_name(shape, counts, disjoint) == name:
            break
    else:
        raise KeyError(name)
    rng = np.random.default_rng(1000 + i)
    n_rows, n_cols = shape
    half = n_rows // 2
    F1 = family(rng, n_rows, n_cols, counts[0], 0, half if disjoint else n_rows)
    F2 = family(rng, n_rows, n_cols, counts[1], half if disjoint else 0, n_rows)
    ones = min(n_rows, 7)
    S = scipy.sparse.coo_matrix((np.ones(ones, dtype=np.int64), (np.arange(ones), np.zeros(ones, dtype=np.int64))), shape=shape)
    return F1, F2, S


@functools.lru_cache(maxsize=None)
def expected(name):
    """The model's answer for a case, computed once: {'O', 'match', 'overlap', 'total', 'shape'}; the arrays are
    read-only."""
    F1, F2, S = case_inputs(name)
    O = overlaps(F1, F2, S.shape)
    match, overlap, total = pairing(O)
    for a in (O, match, overlap):
        a.setflags(write=False)
    return {'O': O, 'match': match, 'overlap': overlap, 'total': total, 'shape': tuple(S.shape)}
