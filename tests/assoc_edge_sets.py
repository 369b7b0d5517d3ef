"""TEST INFRASTRUCTURE: seeded small bool tables (n_rows, n_genomes) for the association screen (csrc/assoc.hip), each
with a column selection, each named after the edge of the kernels it is built to hit. Pure numpy, no GPU:
tests/test_assoc_edges_host.py proves that every generator delivers the property its name claims, so that
tests/test_gpu_assoc_edges.py can rely on it. The yardstick stays tests/assoc_model.py on X[row_map][:, col_map].

Vocabulary. "Under the selection" = in the table view(X, col_map) the device works on: column j of it is genome
col_map[j] of X (col_map None: every genome in order). The signature of a row is that view packed into words of 64
columns; word 0 holds columns 0..63, word 1 starts at column 64. A generator returns None where its edge cannot exist at
the sizes asked for (fits() says the same from the sizes alone).

Selections (selection()):
  none      n_selected = n_genomes, no map
  prefix    the first n_selected entries of a permutation of n_selected + SPARE genomes
  repeats   the same with the genome of column 0 again at columns 1 and 3 (n_selected >= 3); column 64 and the last column
            stay the only ones of their genomes, which the column generators below need
  empty     no column at all (n_selected = 0) of SPARE genomes
Row maps of the resident path (resident_source()): a permutation, and one with repeated entries that leaves source rows
out.
"""
import collections

import numpy as np

N_ROWS = (1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1025)         # the sweep of tests/test_gpu_assoc_edges.py
N_SELECTED = (0, 1, 63, 64, 65, 127, 128, 129, 193)
SPARE = 16                                    # genomes outside a mapped selection (2^16 rows can differ there only)
SELECTIONS = ('none', 'prefix', 'repeats', 'empty')
ROW_MAPS = ('permutation', 'repeats')

Case = collections.namedtuple('Case', 'name X col_map')


def selections_for(n_selected):
    if n_selected == 0:
        return ('empty',)
    return ('none', 'prefix') + (('repeats',) if n_selected >= 3 else ())


def selection(kind, n_selected, rng):
    """(n_genomes, col_map: int32 [n_selected] or None)"""
    if kind == 'none':
        assert n_selected > 0
        return n_selected, None
    if kind == 'empty':
        assert n_selected == 0
        return SPARE, np.zeros(0, dtype=np.int32)
    n_genomes = n_selected + SPARE
    col_map = rng.permutation(n_genomes)[:n_selected].astype(np.int32)
    if kind == 'repeats':
        assert n_selected >= 3
        col_map[1] = col_map[0]
        if n_selected >= 5:
            col_map[3] = col_map[0]
    else:
        assert kind == 'prefix'
    return n_genomes, col_map


def columns(n_genomes, col_map):
    """genome of every column of the selection"""
    return np.arange(n_genomes) if col_map is None else np.asarray(col_map, dtype=np.int64)


def view(X, col_map):
    return X if col_map is None else X[:, np.asarray(col_map, dtype=np.int64)]


def bits_needed(n_rows):
    """columns that tell n_rows rows apart"""
    return max(1, (n_rows - 1).bit_length())


def _own_columns(sel):
    """columns of the selection whose genome no other column has (they can be set one by one)"""
    _, inverse, counts = np.unique(sel, return_inverse=True, return_counts=True)
    return np.flatnonzero(counts[inverse.ravel()] == 1)


def _base(rng, n_rows, n_genomes):
    """one random pattern for every row"""
    return np.tile(rng.random(n_genomes) < 0.5, (n_rows, 1))


def _write_codes(X, genomes, codes):
    """bit b of codes[r] into X[r, genomes[b]]"""
    for b, g in enumerate(genomes):
        X[:, g] = (codes >> b) & 1


def few_patterns(rng, n_rows, n_genomes, col_map, k=5):
    """k random patterns resampled to n_rows rows: many rows are equal and the first row of a block is anywhere."""
    patterns = rng.random((k, n_genomes)) < 0.3
    return patterns[rng.integers(0, k, n_rows)]


def all_distinct(rng, n_rows, n_genomes, col_map):
    """No two rows equal under the selection: a shuffled row number, written into columns spread from the first to the
    last that has a genome of its own; every other genome is the same in all rows."""
    sel = columns(n_genomes, col_map)
    own, bits = _own_columns(sel), bits_needed(n_rows)
    if own.size < bits:
        return None
    carriers = own[np.round(np.linspace(own.size - 1, 0, bits)).astype(np.int64)]       # (the last own column first)
    X = _base(rng, n_rows, n_genomes)
    _write_codes(X, sel[carriers], rng.permutation(n_rows))
    return X


def all_equal(rng, n_rows, n_genomes, col_map):
    """One pattern, not empty under the selection (unless that has no column)."""
    sel = columns(n_genomes, col_map)
    X = _base(rng, n_rows, n_genomes)
    if sel.size:
        X[:, sel[0]] = True
    return X


def all_empty(rng, n_rows, n_genomes, col_map):
    """No row has a selected genome; the genomes outside the selection are random."""
    X = rng.random((n_rows, n_genomes)) < 0.5
    X[:, columns(n_genomes, col_map)] = False
    return X


def differ_in_last_selected_column_only(rng, n_rows, n_genomes, col_map):
    """Two kinds of rows that differ in the last column of the selection and nowhere else: the last bit of the last word
    in use. Row 0 and the last row are of different kinds."""
    sel = columns(n_genomes, col_map)
    if n_rows < 2 or sel.size < 1 or np.count_nonzero(sel == sel[-1]) != 1:
        return None
    X = _base(rng, n_rows, n_genomes)
    X[:, sel[-1]] = rng.random(n_rows) < 0.5
    X[0, sel[-1]], X[-1, sel[-1]] = False, True
    return X


def differ_in_column_64_only(rng, n_rows, n_genomes, col_map):
    """Columns 0..63 (word 0 of the signature) are the same in every row; the rows differ from column 64 on (word 1):
    a shuffled row number modulo 2^bits, bit 0 in column 64, bits = what 127 and the selection leave room for. There are
    min(n_rows, 2^bits) different rows: all of them where the selection has room. A compare that stops after word 0
    makes one block of them."""
    sel = columns(n_genomes, col_map)
    bits = min(bits_needed(n_rows), sel.size - 64)
    if n_rows < 2 or bits < 1:
        return None
    carriers = np.arange(64, 64 + bits)
    if np.setdiff1d(carriers, _own_columns(sel)).size:
        return None
    X = _base(rng, n_rows, n_genomes)
    _write_codes(X, sel[carriers], rng.permutation(n_rows) % (1 << bits))
    return X


def differ_outside_the_selection_only(rng, n_rows, n_genomes, col_map):
    """No two rows equal in the whole table, all rows equal under the selection."""
    outside = np.setdiff1d(np.arange(n_genomes), columns(n_genomes, col_map))
    bits = bits_needed(n_rows)
    if n_rows < 2 or outside.size < bits:
        return None
    X = _base(rng, n_rows, n_genomes)
    _write_codes(X, outside[:bits], rng.permutation(n_rows))
    return X


def empty_rows_at_the_edges(rng, n_rows, n_genomes, col_map):
    """A few patterns, none of them empty under the selection, with empty rows (under the selection; their other genomes
    stay) at row 0, at the last row, at rows 63 and 64 and at one row in ten of the others."""
    sel = columns(n_genomes, col_map)
    if sel.size < 1:
        return None
    X = few_patterns(rng, n_rows, n_genomes, col_map, k=6)
    X[:, sel[0]] |= ~X[:, sel].any(axis=1)
    empty = rng.random(n_rows) < 0.1
    empty[[r for r in (0, 63, 64, n_rows - 1) if r < n_rows]] = True
    X[np.ix_(np.flatnonzero(empty), np.unique(sel))] = False
    return X


GENERATORS = collections.OrderedDict((f.__name__, f) for f in (
    few_patterns, all_distinct, all_equal, all_empty, differ_in_last_selected_column_only, differ_in_column_64_only,
    differ_outside_the_selection_only, empty_rows_at_the_edges))


def fits(name, kind, n_rows, n_selected):
    """Whether generator `name` has a table for selection `kind` at these sizes (None otherwise), from the sizes alone."""
    own = n_selected - {'repeats': 3 if n_selected >= 5 else 2}.get(kind, 0)      # columns with a genome of their own
    if name == 'all_distinct':
        return own >= bits_needed(n_rows)
    if name == 'differ_in_last_selected_column_only':
        return n_rows >= 2 and n_selected >= 1
    if name == 'differ_in_column_64_only':
        return n_rows >= 2 and n_selected >= 65
    if name == 'differ_outside_the_selection_only':
        return n_rows >= 2 and kind != 'none'                # (SPARE genomes or more lie outside a mapped selection)
    if name == 'empty_rows_at_the_edges':
        return n_selected >= 1
    return True


def rng_for(*key):
    return np.random.default_rng([int(k) for k in key])


def cases(n_rows, n_selected, seed=0):
    """Every generator on every selection of n_selected columns, where it fits: Case(name 'generator/selection', X,
    col_map), X of n_rows rows."""
    for kind in selections_for(n_selected):
        for i, (name, gen) in enumerate(GENERATORS.items()):
            rng = rng_for(seed, n_rows, n_selected, SELECTIONS.index(kind), i)
            n_genomes, col_map = selection(kind, n_selected, rng)
            X = gen(rng, n_rows, n_genomes, col_map)
            if X is not None:
                yield Case('%s/%s' % (name, kind), X, col_map)


def resident_source(X, kind, rng):
    """(X_src, row_map int32 [n_rows]): the table of the resident path is X_src[row_map]. 'permutation': that table is
    X itself, its rows scattered over the source; 'repeats': X is the source, entries repeat (the first and the last
    are the same one) and so leave rows of it out."""
    n_rows = X.shape[0]
    if kind == 'permutation':
        row_map = rng.permutation(n_rows).astype(np.int32)
        X_src = np.empty_like(X)
        X_src[row_map] = X
        return X_src, row_map
    assert kind == 'repeats' and n_rows >= 2
    row_map = rng.integers(0, n_rows, n_rows).astype(np.int32)
    row_map[-1] = row_map[0]
    return X, row_map


def target_bits(rng, n_targets, n_selected):
    """bool [n_targets, n_selected]: which columns of the selection each target counts"""
    return rng.random((n_targets, n_selected)) < rng.random((n_targets, 1))


def pack_masks(bits, pad_ones=False):
    """The masks of pgx_assoc for target_bits(): uint64 [n_targets, max(1, ceil(n_selected / 64))], bit j % 64 of word
    j / 64 = column j; the pad bits behind column n_selected - 1 all clear or all set. None without a target."""
    n_targets, n_selected = bits.shape
    if n_targets == 0:
        return None
    words = max(1, -(-n_selected // 64))
    full = np.full((n_targets, words * 64), bool(pad_ones))
    full[:, :n_selected] = bits
    return np.ascontiguousarray(np.packbits(full, axis=1, bitorder='little')).view('<u8')


def bitmap(X, stride_words):
    """The genome-major bitmap of include/pgx.h for the table X: uint64 [n_genomes, stride_words], bit r % 64 of word
    r / 64 = row r."""
    n_rows, n_genomes = X.shape
    full = np.zeros((n_genomes, stride_words * 64), dtype=bool)
    full[:, :n_rows] = X.T
    return np.ascontiguousarray(np.packbits(full, axis=1, bitorder='little')).view('<u8')
