"""tests/assoc_edge_sets.py delivers what its names claim (no GPU): every generator, on every selection and at every
size of the sweep of tests/test_gpu_assoc_edges.py, is checked against tests/assoc_model.py for the property it is named
after, so that a later edit cannot turn an edge case into an ordinary one unnoticed."""
import numpy as np
import pytest

import assoc_edge_sets as es
import assoc_model

SIZES = [(n, s) for n in es.N_ROWS for s in es.N_SELECTED]


def made(name, kind, n_rows, n_selected, seed=0):
    """(X, col_map, V = the table under the selection) of one generator, or None"""
    rng = es.rng_for(seed, n_rows, n_selected, 7)
    n_genomes, col_map = es.selection(kind, n_selected, rng)
    X = es.GENERATORS[name](rng, n_rows, n_genomes, col_map)
    if X is None:
        return None
    assert X.dtype == bool and X.shape == (n_rows, n_genomes)
    return X, col_map, es.view(X, col_map)


def every(name):
    """every table generator `name` makes over the sweep; where it makes none, fits() says so"""
    for n_rows, n_selected in SIZES:
        for kind in es.selections_for(n_selected):
            got = made(name, kind, n_rows, n_selected)
            assert (got is not None) == es.fits(name, kind, n_rows, n_selected), (name, kind, n_rows, n_selected)
            if got is not None:
                yield (n_rows, n_selected, kind) + got


def n_blocks(V):
    return assoc_model.blocks(V)[1].size


def test_the_selections():
    for n_selected in es.N_SELECTED:
        kinds = es.selections_for(n_selected)
        assert kinds == (('empty',) if n_selected == 0 else ('none', 'prefix', 'repeats') if n_selected >= 3 else ('none', 'prefix'))
        for kind in kinds:
            n_genomes, col_map = es.selection(kind, n_selected, es.rng_for(1, n_selected))
            sel = es.columns(n_genomes, col_map)
            assert sel.size == n_selected and n_genomes > 0
            assert (col_map is None) == (kind == 'none')
            if col_map is not None:
                assert col_map.dtype == np.int32 and col_map.min(initial=0) >= 0 and col_map.max(initial=0) < n_genomes
                assert n_genomes - np.unique(sel).size >= es.SPARE                      # genomes outside the selection
            if kind == 'none':
                assert n_genomes == n_selected
            if kind == 'prefix':
                assert np.unique(sel).size == n_selected
                assert n_selected == 1 or not np.array_equal(sel, np.sort(sel))           # a permutation, not in order
            if kind == 'repeats':
                assert np.unique(sel).size < n_selected and sel[1] == sel[0]              # really a repeat
                assert np.count_nonzero(sel == sel[-1]) == 1
                if n_selected > 64:
                    assert np.count_nonzero(sel == sel[64]) == 1


def test_the_sweep_has_every_generator_at_every_row_count():
    for n_rows in es.N_ROWS:
        names = {c.name.split('/')[0] for s in es.N_SELECTED for c in es.cases(n_rows, s)}
        want = set(es.GENERATORS)
        if n_rows < 2:
            want -= {'differ_in_last_selected_column_only', 'differ_in_column_64_only', 'differ_outside_the_selection_only'}
        assert names == want, n_rows
    kinds = {c.name.split('/')[1] for s in es.N_SELECTED for c in es.cases(33, s)}
    assert kinds == set(es.SELECTIONS)
    for a, b in zip(es.cases(65, 129), es.cases(65, 129)):                              # seeded: the same every time
        assert a.name == b.name and np.array_equal(a.X, b.X) and np.array_equal(a.col_map, b.col_map)


def test_few_patterns():
    for n_rows, n_selected, kind, X, col_map, V in every('few_patterns'):
        assert n_blocks(V) <= 5
    X = es.few_patterns(es.rng_for(3), 4097, 200, None, k=40)
    block_of_row, rep_row = assoc_model.blocks(X)
    assert rep_row.size == 40 and rep_row.max() > 40                   # the first row of a block is anywhere
    assert np.bincount(block_of_row).min() > 1


def test_all_distinct():
    seen = 0
    for n_rows, n_selected, kind, X, col_map, V in every('all_distinct'):
        assert n_blocks(V) == n_rows
        assert 2 ** min(n_selected, 62) >= n_rows
        seen += 1
    assert seen > 150
    for n_rows in (32, 33, 2049, 65535, 65536, 65537):                 # the sizes the device tests use it at
        X = es.all_distinct(es.rng_for(n_rows), n_rows, 17, None)
        b, rep = assoc_model.blocks(X)
        assert np.array_equal(b, np.arange(n_rows)) and np.array_equal(rep, np.arange(n_rows))
    assert es.all_distinct(es.rng_for(0), 257, 8, None) is None        # 2^8 < 257


def test_all_equal_and_all_empty():
    for n_rows, n_selected, kind, X, col_map, V in every('all_equal'):
        assert n_blocks(V) == 1 and V.any(axis=1).all() == (n_selected > 0)
        assert assoc_model.blocks_drop_empty(V)[1].size == (1 if n_selected else 0)
    for n_rows, n_selected, kind, X, col_map, V in every('all_empty'):
        assert not V.any() and n_blocks(V) == 1
        b, rep = assoc_model.blocks_drop_empty(V)
        assert (b == -1).all() and rep.size == 0
        if col_map is not None and n_rows >= 31:
            assert X.any()                                             # the rows are empty under the selection only


def test_differ_in_last_selected_column_only():
    for n_rows, n_selected, kind, X, col_map, V in every('differ_in_last_selected_column_only'):
        assert n_blocks(V) == 2 and n_blocks(V[:, :-1]) == 1
        assert not V[0, -1] and V[-1, -1]


def test_differ_in_column_64_only():
    pairwise_distinct = 0
    for n_rows, n_selected, kind, X, col_map, V in every('differ_in_column_64_only'):
        assert n_selected >= 65
        assert n_blocks(V[:, :64]) == 1                                # word 0 is equal ...
        assert n_blocks(V[:, 64:128]) == n_blocks(V) == min(n_rows, 2 ** min(n_selected - 64, 20))   # ... word 1 differs
        assert n_blocks(V[:, 128:]) == 1
        assert V[:, 64].any() and not V[:, 64].all()
        pairwise_distinct += n_blocks(V) == n_rows
    assert pairwise_distinct >= 3 * 4 * 11                             # wherever n_selected >= 127: every row count but 1


def test_differ_outside_the_selection_only():
    for n_rows, n_selected, kind, X, col_map, V in every('differ_outside_the_selection_only'):
        assert col_map is not None
        assert n_blocks(X) == n_rows and n_blocks(V) == 1


def test_empty_rows_at_the_edges():
    for n_rows, n_selected, kind, X, col_map, V in every('empty_rows_at_the_edges'):
        empty = ~V.any(axis=1)
        for r in (0, 63, 64, n_rows - 1):
            assert r >= n_rows or empty[r]
        if n_rows >= 255:
            assert 4 < empty.sum() < n_rows // 4 and not empty[1:63].all()              # plus a sprinkle, not everything
            inside_last_wave = empty[(n_rows - 1) // 64 * 64:]
            assert inside_last_wave[-1]
        b, rep = assoc_model.blocks_drop_empty(V)
        assert np.array_equal(b < 0, empty) and (rep.size == 0 or not empty[rep].any())
        assert n_blocks(V) == rep.size + 1                             # the empty rows are one more block
        if col_map is not None and n_rows >= 31:
            assert X[empty].any()                                      # empty under the selection, not in the table


def test_blocks_drop_empty_is_blocks_of_the_rows_that_are_left():
    rng = es.rng_for(9)
    X = es.empty_rows_at_the_edges(rng, 257, 70, None)
    b, rep = assoc_model.blocks_drop_empty(X)
    kept = np.flatnonzero(X.any(axis=1))
    bk, repk = assoc_model.blocks(X[kept])
    assert np.array_equal(b[kept], bk) and np.array_equal(rep, kept[repk]) and (np.delete(b, kept) == -1).all()
    assert np.array_equal(X[rep][b[kept]], X[kept])


@pytest.mark.parametrize('kind', es.ROW_MAPS)
def test_row_maps(kind):
    for n_rows in es.N_ROWS[1:]:
        rng = es.rng_for(2, n_rows)
        X = es.all_distinct(rng, n_rows, 20, None)
        X_src, row_map = es.resident_source(X, kind, rng)
        assert row_map.dtype == np.int32 and row_map.shape == (n_rows,) and X_src.shape == X.shape
        assert row_map.min() >= 0 and row_map.max() < n_rows
        if kind == 'permutation':
            assert np.array_equal(np.sort(row_map), np.arange(n_rows)) and np.array_equal(X_src[row_map], X)
            assert n_rows < 31 or not np.array_equal(row_map, np.arange(n_rows))
        else:
            assert np.unique(row_map).size < n_rows and row_map[0] == row_map[-1]        # repeats, and rows left out
            assert n_blocks(X_src[row_map]) == np.unique(row_map).size


def test_masks_and_bitmap_layout():
    rng = es.rng_for(4)
    for n_selected in es.N_SELECTED:
        bits = es.target_bits(rng, 3, n_selected)
        clear, ones = es.pack_masks(bits), es.pack_masks(bits, pad_ones=True)
        words = max(1, (n_selected + 63) // 64)
        assert clear.dtype == np.uint64 and clear.shape == ones.shape == (3, words)
        for t in range(3):
            for j in range(words * 64):
                want = bool(bits[t, j]) if j < n_selected else False
                assert bool((int(clear[t, j // 64]) >> (j % 64)) & 1) == want
                assert bool((int(ones[t, j // 64]) >> (j % 64)) & 1) == (want or j >= n_selected)
        assert (clear != ones).any() == (n_selected % 64 != 0 or n_selected == 0)
    assert es.pack_masks(es.target_bits(rng, 0, 65)) is None
    X = rng.random((130, 5)) < 0.5
    bm = es.bitmap(X, 16)
    assert bm.dtype == np.uint64 and bm.shape == (5, 16)
    for r in range(130):
        for g in range(5):
            assert bool((int(bm[g, r // 64]) >> (r % 64)) & 1) == bool(X[r, g])
    assert not bm[:, 3:].any() and not (bm[:, 2] >> np.uint64(2)).any()
