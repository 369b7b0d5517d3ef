"""TEST INFRASTRUCTURE: a plain-numpy restatement (one thread) of the rules of the association screen as the device
states them (include/pgx.h, "The association screen"; pangenomix_amd/csrc/assoc.hip), for table sizes where
no fixture of the reference exists. tests/test_assoc_host.py checks it against every fixture, so it is a fair yardstick.

    blocks       two rows are the same block iff they are present in the same columns; blocks are numbered by their
                 first row; all empty rows form one block
    contingency  TP[r] = columns where row r is present and the target is non-zero (a NaN counts); FP = incidence - TP;
                 FN = target.sum() - TP; TN = n_samples - TP - FP - FN
    selection    half = max_features // 2; rows by LOR descending, stable, NaN last; first half + last half of that order
"""
import numpy as np


def dense(rows, cols, shape):
    X = np.zeros(shape, dtype=bool)
    X[np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)] = True
    return X


def blocks(X):
    """(block_of_row int64 [n_rows], rep_row int64 [n_blocks]) of the bool table X."""
    X = np.asarray(X) != 0
    n_rows = X.shape[0]
    if n_rows == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    packed = np.ascontiguousarray(np.packbits(X, axis=1)) if X.shape[1] else np.zeros((n_rows, 1), dtype=np.uint8)
    keys = packed.view(np.dtype((np.void, packed.shape[1]))).ravel()
    _, first, inverse = np.unique(keys, return_index=True, return_inverse=True)
    rank = np.empty(first.size, dtype=np.int64)
    rank[np.argsort(first, kind='stable')] = np.arange(first.size)      # unique key -> block number (by first row)
    return rank[inverse.ravel()], np.sort(first).astype(np.int64)


def blocks_drop_empty(X):
    """blocks() of the table without its empty rows (PGX_ASSOC_DROP_EMPTY), in the row numbers of the whole table:
    block_of_row is -1 for an empty row, rep_row holds rows of X."""
    X = np.asarray(X) != 0
    kept = np.flatnonzero(X.any(axis=1))
    b, rep = blocks(X[kept])
    block_of_row = np.full(X.shape[0], -1, dtype=np.int64)
    block_of_row[kept] = b
    return block_of_row, kept[rep].astype(np.int64)


def definitions(block_of_row, n_blocks):
    """[rows of block b, ascending] for every block; rows of block -1 belong to none."""
    block_of_row = np.asarray(block_of_row, dtype=np.int64)
    out = [[] for _ in range(int(n_blocks))]
    for r, b in enumerate(block_of_row.tolist()):
        if b >= 0:
            out[b].append(r)
    return out


def contingency(X, target):
    """float64 (n_rows, 4) of the bool table X against one target vector."""
    X = np.asarray(X) != 0
    target = np.asarray(target)
    n_samples = X.shape[1]
    positives = float(target.sum())
    incidence = X.sum(axis=1, dtype=np.int64)
    TPs = (X & (target != 0)[None, :]).sum(axis=1, dtype=np.int64)
    FPs = incidence - TPs
    FNs = positives - TPs
    TNs = n_samples - TPs - FPs - FNs
    out = np.zeros((X.shape[0], 4))
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = TPs, FPs, FNs, TNs
    return out


def adjusted_lor(c):
    with np.errstate(all='ignore'):
        pr = (c[:, 0] + c[:, 2]) / c.sum(axis=1, dtype='float')
        nr = 1.0 - pr
        return np.log2(((c[:, 0] + pr) * (c[:, 3] + nr)) / ((c[:, 1] + nr) * (c[:, 2] + pr)))


def select(lors, max_features):
    """Row positions the LOR filter keeps (an explicit three-part key per row instead of a sort routine's tie rule)."""
    lors = np.asarray(lors, dtype=np.float64)
    half = int(max_features) // 2
    nan = lors != lors
    order = np.lexsort((np.arange(lors.size), np.where(nan, 0.0, -lors), nan))     # (the last key is the primary one)
    return order[:half].tolist() + order[order.size - half:].tolist()


def screen(X, phenotype, min_freq=3, max_features=10000):
    """One drug's screen on the bool table X (features x genomes): phenotype holds one value per genome, NaN = none.
    Returns (genomes kept, rows kept, block_of_row over the kept rows, rep_row, rows of the block table selected)."""
    X = np.asarray(X) != 0
    phenotype = np.asarray(phenotype, dtype=np.float64)
    genomes = np.flatnonzero(phenotype == phenotype)
    sub = X[:, genomes]
    kept = np.flatnonzero(sub.any(axis=1))
    sub = sub[kept]
    block_of_row, rep_row = blocks(sub)
    B = sub[rep_row]
    rows = np.arange(B.shape[0])
    if min_freq > 0:
        rows = np.flatnonzero(B.sum(axis=1) >= min_freq)
    if rows.size > max_features:
        lors = adjusted_lor(contingency(B[rows], phenotype[genomes]))
        rows = rows[np.asarray(select(lors, max_features), dtype=np.int64)]
    return genomes, kept, block_of_row, rep_row, rows


def load_table_fixture(path):
    """A tests/golden/assoc/table_*.npz (written by tests/golden/make_golden_assoc.py from a run of the reference)."""
    d = np.load(path)
    out = {k: d[k] for k in d.files}
    out['rows'], out['cols'] = d['rows'].astype(np.int64), d['cols'].astype(np.int64)
    out['shape'] = tuple(int(x) for x in d['shape'])
    out['dtype'] = str(d['dtype'])
    out['types'] = [str(x) for x in d['types']]
    return out
