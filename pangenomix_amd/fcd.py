"""
Formal concept decomposition of a binary table on MI355X.

Mirror of the reference's fcd.py: `formal_concept_decomposition` (Algorithm 2 of
https://doi.org/10.1016/j.jcss.2009.05.002) greedily covers the gene x genome (or allele x genome) table with all-ones
blocks ("concepts": a set of rows x a set of genomes) and returns the factorisation W, H and the concept list F -- how a
pangenome is broken into core / clade / strain-specific blocks. Same names, positional order and defaults, and the same
F (concepts, their order, container types); `ctx` is the only addition.

Every step of the greedy loop is "for each genome column, count the ones among the rows still in play": a masked
popcount over the genome-major bitmap libpgx builds and keeps resident (pangenomix_amd/csrc/fcd.hip). The
reference copies a dense int64 block with np.ix_ and sums it. The table goes to the device as coordinates and is never
densified here; the shuffle of `seed` is numpy's own, on the host. There is no CPU fallback.

The helpers around it (decompose / encode / sort / load / save) are plain numpy, as in the reference;
`compute_concept_coverage` clears the concepts' blocks on the device with the kernel the decomposition uses.

`compute_concept_list_similarity` is the reference's host loop unless it is given a context: then the two lists become
row and column bit masks on the device, the cells every pair of concepts shares are an AND + popcount product, and the
greedy pairing runs there too (pangenomix_amd/csrc/fcd_match.hip). `match_concept_lists` returns that pairing, which the
reference throws away, and `concept_overlaps` the whole overlap matrix.
"""

from __future__ import print_function

import numpy as np
import pandas as pd
import scipy.sparse

from . import _native, sparse_utils

_NOT_BINARY = 'formal_concept_decomposition needs a binary (0/1) table'
_DUPLICATES = 'formal_concept_decomposition needs a table without duplicate entries'


def _table(S):
    """(rows, cols, shape, resident) of the table's ones (int64 coordinates), from a dense 2-D array of 0/1 values (any
    integer, bool or float dtype), a scipy.sparse matrix or a LightSparseDataFrame (read through their coordinates, never
    densified). Anything that is not 0/1 raises ValueError. `resident` is the pipeline's hand-off record of a table
    returned by build_cds_pangenome(), or None."""
    resident = None
    if isinstance(S, sparse_utils.LightSparseDataFrame):
        resident = getattr(S, '_pgx_resident', None)
        if resident is not None and not (resident['shape'] == tuple(S.shape) and resident['data'] is S.data
                                         and resident['nnz'] == int(S.data.nnz) and 'row_cluster' in resident):
            resident = None                  # (no longer the table the pipeline returned)
        S = S.data
    if scipy.sparse.issparse(S):
        coo = S if S.format == 'coo' else S.tocoo()
        data = np.asarray(coo.data)
        try:
            ones = data == 1
            ok = np.all(ones | (data == 0))
        except TypeError:
            raise ValueError(_NOT_BINARY)
        if not ok:
            raise ValueError(_NOT_BINARY)
        rows, cols = np.asarray(coo.row, dtype=np.int64), np.asarray(coo.col, dtype=np.int64)
        if not np.all(ones):                 # (stored zeros are absent cells)
            rows, cols, resident = rows[ones], cols[ones], None
        return rows, cols, tuple(int(x) for x in coo.shape), resident
    X = np.asarray(S)
    if X.ndim != 2:
        raise ValueError('formal_concept_decomposition takes a 2-D table')
    try:
        ones = np.asarray(X == 1, dtype=bool)
        ok = np.all(ones | np.asarray(X == 0, dtype=bool))
    except TypeError:
        raise ValueError(_NOT_BINARY)
    if not ok:
        raise ValueError(_NOT_BINARY)
    rows, cols = np.nonzero(ones)
    return rows.astype(np.int64), cols.astype(np.int64), X.shape, None


def _dim_factors(n_rows, n_cols):
    """The reference's dim_balance factor of every step, `(len(concept_columns) + 1) ** dim_coeff` with its own
    expressions (numpy float64 throughout; one column gives its inf / nan), so that the device's single multiply
    reproduces the reference's scores bit for bit."""
    dim_coeff = np.log(n_rows) / np.log(n_cols)
    return np.array([(k + 1) ** dim_coeff for k in range(n_cols)], dtype=np.float64)


def _concepts(S, limit=None, overlap=False, dim_balance=False, seed=None, ctx=None):
    """(F in discovery order, shape, info): the device part of formal_concept_decomposition. info: 'left' (ones uncovered
    after each concept), 'steps', 'ones_total', 'ones_left'."""
    rows, cols, (n_rows, n_cols), resident = _table(S)
    ctx = ctx or _native.default_context()
    row_shuffle = col_shuffle = None
    if seed is not None:     # the reference's shuffle, by numpy itself: the global generator ends where it leaves it
        np.random.seed(seed)
        row_shuffle = np.arange(n_rows); np.random.shuffle(row_shuffle)
        col_shuffle = np.arange(n_cols); np.random.shuffle(col_shuffle)
    if limit is None:
        limit = n_rows * n_cols
    limit = max(int(limit), 0)
    info = {'left': np.zeros(0, dtype=np.uint64), 'steps': 0, 'ones_total': int(rows.size), 'ones_left': int(rows.size)}
    if n_rows == 0 or n_cols == 0:
        return [], (n_rows, n_cols), info
    factors = _dim_factors(n_rows, n_cols) if dim_balance and not overlap else None
    out = None
    if resident is not None and resident['ctx'] is ctx:
        # the pipeline left this table's bitmap on the device: nothing of the table travels, the device copies (and
        # shuffles) it into its own workspace
        row_map = resident['row_cluster'] if row_shuffle is None else resident['row_cluster'][row_shuffle]
        try:
            out = ctx.fcd_resident(resident['token'], row_map, col_shuffle, n_cols, limit, overlap, factors)
        except _native.PgxError as e:
            if getattr(e, 'status', 0) != -1:            # (PGX_ERR_INVALID: another pipeline has replaced it since --
                raise                                    #  the coordinates go up instead)
    if out is None:
        if row_shuffle is not None:          # U = S[row_shuffle, :][:, col_shuffle]: the ones move, nothing is densified
            inv_r = np.empty(n_rows, dtype=np.int64); inv_r[row_shuffle] = np.arange(n_rows)
            inv_c = np.empty(n_cols, dtype=np.int64); inv_c[col_shuffle] = np.arange(n_cols)
            rows, cols = inv_r[rows], inv_c[cols]
        out, dup = ctx.fcd(rows, cols, n_rows, n_cols, limit, overlap, factors)
        if dup:
            raise ValueError(_DUPLICATES)
    ro, co = out['row_offsets'].astype(np.int64), out['col_offsets'].astype(np.int64)
    F = []
    for i in range(ro.size - 1):
        x, y = out['rows'][ro[i]:ro[i + 1]], out['cols'][co[i]:co[i + 1]]
        if seed is None:
            F.append((tuple(x.tolist()), tuple(y.tolist())))
        else:                                # un-shuffled as the reference does it: lists of the shuffles' entries
            F.append((list(row_shuffle[x]), list(col_shuffle[y])))
    info = {k: out[k] for k in ('left', 'steps', 'ones_total', 'ones_left')}
    return F, (n_rows, n_cols), info


def formal_concept_decomposition(S, limit=None, sort_components=True, overlap=False, dim_balance=False, seed=None,
                                 verbose=False, ctx=None):
    """Greedy cover of the binary table S with all-ones blocks, largest gain first.

    S               : dense 2-D array of 0/1 (integer, bool or float), scipy.sparse matrix or LightSparseDataFrame. The
                      gene table returned by build_cds_pangenome() is read from the bitmap the pipeline left on the
                      device (which is not modified), without uploading it.
    limit           : maximum number of concepts; None = a complete decomposition
    sort_components : sort the concepts by size (rows x columns), largest first; False keeps the order of discovery
    overlap         : allow concepts to cover a one more than once; then (W @ H > 0) == S rather than W @ H == S
    dim_balance     : balance the propensity to grow a block in either dimension (ignored under overlap)
    seed            : shuffle rows and columns (np.random.seed(seed), two np.random.shuffle) for another factorisation
    verbose         : print 'Components found: n | Coverage: x' once per concept
    ctx             : optional pangenomix_amd._native.Context (default: process-wide)

    One deliberate deviation: with `seed` AND `overlap` the reference takes the overlap terms and the row update from
    the table as it was before the shuffle, under the row and column numbers after it, so what it returns there are not
    all-ones blocks of S. Here the shuffled table is read throughout.

    Returns (W, H, F): F is the list of concepts ((rows), (columns)) -- tuples, or lists when `seed` is given; rows
    ascending in the (shuffled) table, columns in the order they joined -- and W (rows x concepts), H (concepts x
    columns) are the int arrays of decompose_from_concepts(). Raises RuntimeError (PgxError) where the reference would
    loop for ever: a concept that clears nothing.
    """
    F, shape, info = _concepts(S, limit, overlap, dim_balance, seed, ctx)
    if verbose:
        total = float(info['ones_total'])
        for i, left in enumerate(info['left']):
            print('Components found:', i + 1, '|', 'Coverage:', 1.0 - np.int64(left) / total)
    if sort_components:
        F = sort_concepts_by_size(F)
    W, H = _decompose(shape, F)
    return W, H, F


def _decompose(shape, F):
    m, n = shape
    W = np.zeros((m, len(F)), dtype=int)
    H = np.zeros((len(F), n), dtype=int)
    for i, (x_terms, y_terms) in enumerate(F):
        W[np.asarray(x_terms, dtype=np.int64), i] = 1
        H[i, np.asarray(y_terms, dtype=np.int64)] = 1
    return W, H


def decompose_from_concepts(S, F):
    """(W, H) int arrays of the concepts F of the table S (only its shape is used): W[x, i] = 1 for the rows x of
    concept i, H[i, y] = 1 for its columns y."""
    return _decompose(S.shape, F)


def encode_from_concepts(F):
    """H of decompose_from_concepts() without the table: as many columns as the largest column index needs."""
    n = 0
    for concept in F:
        n = max(max(concept[1]), n)
    H = np.zeros(shape=(len(F), n + 1), dtype=int)
    for i, concept in enumerate(F):
        H[i, np.asarray(concept[1], dtype=np.int64)] = 1
    return H


def _match(F1, F2, shape, ctx, matrix):
    n_rows, n_cols = (int(x) for x in shape)
    lists = _flatten(F1) + _flatten(F2)
    for name, bound, parts in (('row', n_rows, lists[0::4]), ('column', n_cols, lists[2::4])):
        for idx in parts:
            if idx.size and (idx.min() < 0 or idx.max() >= bound):
                raise IndexError('a concept names a %s outside the table' % name)
    ctx = ctx or _native.default_context()
    return ctx.fcd_match(n_rows, n_cols, *lists, matrix=matrix)


def match_concept_lists(F1, F2, shape, ctx=None):
    """The pairing compute_concept_list_similarity makes and throws away, on the device: (match, overlap, total) with
    match[i] = the concept of F2 paired with F1[i] and overlap[i] = the cells the two share (int64 arrays of
    min(len(F1), len(F2)) entries), total = sum(overlap) as a Python int. Every concept of F1, in order, takes the
    unmatched concept of F2 it shares the most cells with, the lowest index among equals; sharing nothing still takes
    one. shape = (rows, columns) of the table; an index outside it raises IndexError. A concept is a set: an index
    listed twice counts once."""
    match, overlap, total, _ = _match(F1, F2, shape, ctx, False)
    return match, overlap.astype(np.int64), total


def concept_overlaps(F1, F2, shape, ctx=None):
    """O[i][j] = the cells F1[i] and F2[j] share (rows in common x columns in common): len(F1) x len(F2), int64."""
    return _match(F1, F2, shape, ctx, True)[3].astype(np.int64)


def _ones(S):
    """the denominator of the similarity score, the reference's expression"""
    if isinstance(S, sparse_utils.LightSparseDataFrame):
        return float(np.sum(S.data.data))
    return float(np.sum(S))


def compute_concept_list_similarity(F1, F2, S, ctx=None):
    """How alike two decompositions are: every concept of F1, in order, is paired with the unmatched concept of F2 it
    shares the most cells with (the first among equals); the score is the cells shared by the pairs over the ones of S.

    Without `ctx` this is the reference's double loop over pairs of Python sets, on the host. With a
    pangenomix_amd._native.Context the pairing runs on the device (match_concept_lists, which also returns the pairs);
    the division stays Python's, so the score has the same bits and an all-zero S raises ZeroDivisionError either way.
    On that path S may also be a LightSparseDataFrame, and an index outside S raises IndexError."""
    if ctx is not None:
        return _match(F1, F2, S.shape, ctx, False)[2] / _ones(S)

    def shared(C1, C2):
        return len(set(C1[0]).intersection(C2[0])) * len(set(C1[1]).intersection(C2[1]))

    unmatched = list(range(len(F2)))
    total, i = 0, 0
    while len(unmatched) > 0 and i < len(F1):
        best_match, best = None, -1
        for j in unmatched:
            cells = shared(F1[i], F2[j])
            if cells > best:
                best, best_match = cells, j
        unmatched.remove(best_match)
        total += best
        i += 1
    return total / float(np.sum(S))


def _flatten(F):
    """concepts -> (rows int64, row offsets, cols int64, col offsets)"""
    ro, co = np.zeros(len(F) + 1, dtype=np.uint64), np.zeros(len(F) + 1, dtype=np.uint64)
    xs, ys = [], []
    for i, (x, y) in enumerate(F):
        xs.append(np.asarray(x, dtype=np.int64).reshape(-1))
        ys.append(np.asarray(y, dtype=np.int64).reshape(-1))
        ro[i + 1], co[i + 1] = ro[i] + xs[-1].size, co[i] + ys[-1].size
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)   # noqa: E731
    return cat(xs), ro, cat(ys), co


def compute_concept_coverage(S, F, plot=False, log_rate=50, ctx=None):
    """coverage[i] = the fraction of the ones of S that the first i concepts of F cover (float64, len(F) + 1 values).
    The concepts' blocks are cleared one after the other on the device (the decomposition's own kernel, which returns
    how many ones a block cleared); the running fraction is formed on the host with the reference's expressions. S as
    for formal_concept_decomposition. A concept is a set of rows and a set of columns: an index listed twice in one
    concept raises ValueError. plot=True draws the curve with matplotlib (the reference's seaborn tsplot is gone)."""
    rows, cols, (n_rows, n_cols), _ = _table(S)
    xs, ro, ys, co = _flatten(F)
    for name, idx, off, bound in (('row', xs, ro, n_rows), ('column', ys, co, n_cols)):
        if idx.size and (idx.min() < 0 or idx.max() >= bound):
            raise IndexError('a concept names a %s outside the table' % name)
        for i in range(len(F)):
            part = idx[int(off[i]):int(off[i + 1])]
            if np.unique(part).size != part.size:
                raise ValueError('a concept lists a %s twice' % name)
    ctx = ctx or _native.default_context()
    cleared, ones, dup = ctx.fcd_coverage(rows, cols, n_rows, n_cols, xs, ro, ys, co)
    if dup:
        raise ValueError(_DUPLICATES)
    total_relations = float(ones)
    uncovered_relations = total_relations
    coverage = np.zeros(len(F) + 1)
    with np.errstate(invalid='ignore', divide='ignore'):
        for i in range(len(F)):
            if log_rate > 0 and (i + 1) % log_rate == 0:
                print('Factor', i + 1, 'of', len(F))
            uncovered_relations -= np.int64(cleared[i])
            coverage[i + 1] = 1.0 - uncovered_relations / total_relations
    if plot:
        import matplotlib.pyplot as plt
        ax = plt.gca()
        ax.plot(np.arange(len(F) + 1), coverage)
        ax.axhline(y=1.0, color='k', linestyle='--')
        ax.set_title('Relationships covered vs. Number of binary ICs')
        ax.set_xlabel('# binary ICs')
        ax.set_ylabel('fraction of relationships covered')
    return coverage


def sort_concepts_by_size(F):
    """The concepts by size (rows x columns), largest first; equal sizes keep their order."""
    return sorted(F, key=lambda f: len(f[0]) * len(f[1]), reverse=True)


def load_formal_concepts(path, sort_components=False):
    """The concept list of a file written by save_formal_concepts (tuples of int)."""
    F = []
    with open(path, 'r') as f:
        for line in f:
            _, x_out, y_out = line.split('|')
            F.append((tuple(int(x) for x in x_out.split(',')), tuple(int(y) for y in y_out.split(','))))
    if sort_components:
        F = sort_concepts_by_size(F)
    return F


def save_formal_concepts(F, path):
    """One line per concept, '<i>|<rows, comma separated>|<columns>', no newline after the last."""
    lines = [str(i) + '|' + ','.join(map(str, x_terms)) + '|' + ','.join(map(str, y_terms))
             for i, (x_terms, y_terms) in enumerate(F)]
    with open(path, 'w+') as f:
        f.write('\n'.join(lines))


def save_formal_concepts_full(F, path_W, path_H, path_F, ref_table):
    """The concepts (path_F) and the labelled loading / encoding matrices W (path_W) and H (path_H) as CSV, zeros
    written as empty cells. ref_table: the DataFrame that was decomposed."""
    W, H = decompose_from_concepts(ref_table.values, F)
    labels = ['FCD_' + str(x) for x in range(len(H))]
    pd.DataFrame(W, index=ref_table.index, columns=labels).replace(0, np.nan).to_csv(path_W)
    pd.DataFrame(H, index=labels, columns=ref_table.columns).replace(0, np.nan).to_csv(path_H)
    save_formal_concepts(F, path_F)
