"""The association screen's kernels (csrc/assoc.hip) at their edges, against the numpy model (tests/assoc_model.py) on
the tables of tests/assoc_edge_sets.py (tests/test_assoc_edges_host.py proves that each table has the edge it is named
after). Every comparison is exact: incidence, tp, block_of_row, rep_row and n_blocks are integers.

Everything runs twice, the second time with PGX_ASSOC_NARROW_HASH: 3 bits of hash, every probe collides (so the
word-for-word compare of the signatures decides), the probe sequence starts 4 slots before the end of the block table (so
it wraps), same output byte for byte."""
import numpy as np
import pytest

import assoc_edge_sets as es
import assoc_model

pytestmark = pytest.mark.gpu

MODES = ('blocks', 'drop_empty', 'no_blocks')
N_TARGETS = (0, 1, 3)
KEYS = ('incidence', 'tp', 'block_of_row', 'rep_row')


def flags_of(mode):
    return {'blocks': mode != 'no_blocks', 'drop_empty': mode == 'drop_empty'}


def expected(V, tbits, mode):
    """What the device must return for the table V (rows x selected columns) and the targets tbits (bool [n_targets,
    n_selected])."""
    want = {'incidence': V.sum(axis=1).astype(np.uint32),
            'tp': (V[None, :, :] & tbits[:, None, :]).sum(axis=2).astype(np.uint32), 'block_of_row': None, 'rep_row': None}
    if mode != 'no_blocks':
        b, rep = assoc_model.blocks_drop_empty(V) if mode == 'drop_empty' else assoc_model.blocks(V)
        want['block_of_row'], want['rep_row'] = b.astype(np.int32), rep.astype(np.int32)
    return want


def same(got, want, what):
    for k in KEYS:
        if want[k] is None:
            assert got[k] is None, (what, k)
        else:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
            assert np.array_equal(got[k], want[k]), (what, k)


def same_bytes(a, b, what):
    for k in KEYS:
        assert (a[k] is None) == (b[k] is None), (what, k)
        assert a[k] is None or (a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes()), (what, k)


def twice(call, what):
    """call(narrow_hash) -> result dict, without and with the narrow hash: the same bytes; returns the first."""
    plain, narrow = call(False), call(True)
    same_bytes(plain, narrow, (what, 'narrow hash'))
    return plain


def coo(X):
    return np.nonzero(X)


def make_resident(ctx, X_src):
    """The table X_src as a pipeline leaves it on the device: one record per entry, rows = cluster numbers."""
    r, c = coo(X_src)
    G, S = X_src.shape
    return ctx.bitmap_from_clusters(r, np.arange(r.size), c.astype(np.uint32), np.arange(S), G, S)


# ---------------------------------------------------------------------------------------------------------------------
# the size sweep: n_rows x n_selected x generators x selections, through the three entry points

@pytest.mark.parametrize('n_rows', es.N_ROWS)
def test_sweep_host_entry(n_rows, gpu_ctx):
    """Context.assoc (host COO): every case of the sweep in all three flag settings; 0, 1 and 3 masks take turns."""
    turn = 0
    for n_selected in es.N_SELECTED:
        for case in es.cases(n_rows, n_selected):
            V, (r, c) = es.view(case.X, case.col_map), coo(case.X)
            tbits = es.target_bits(es.rng_for(5, n_rows, turn), N_TARGETS[turn % 3], n_selected)
            masks = es.pack_masks(tbits)
            turn += 1
            for mode in MODES:
                what = (case.name, n_rows, n_selected, mode)
                got = twice(lambda narrow: gpu_ctx.assoc(r, c, n_rows, case.X.shape[1], case.col_map, masks,
                                                         narrow_hash=narrow, **flags_of(mode))[0], what)
                same(got, expected(V, tbits, mode), what)
    assert turn >= 100


@pytest.mark.parametrize('n_rows', es.N_ROWS)
def test_sweep_resident_entry(n_rows, gpu_ctx):
    """assoc_resident: every case of the sweep behind a row map -- a permutation and one with repeats, which leaves rows
    of the resident table out -- taking turns with the flag settings and the number of masks."""
    turn = 0
    for n_selected in es.N_SELECTED:
        for case in es.cases(n_rows, n_selected):
            kind = es.ROW_MAPS[turn % 2] if n_rows >= 2 else 'permutation'
            mode = MODES[(turn // 2) % 3]
            rng = es.rng_for(6, n_rows, turn)
            X_src, row_map = es.resident_source(case.X, kind, rng)
            V = es.view(X_src[row_map], case.col_map)
            tbits = es.target_bits(rng, N_TARGETS[(turn // 6) % 3], n_selected)
            masks = es.pack_masks(tbits)
            turn += 1
            token = make_resident(gpu_ctx, X_src)
            what = (case.name, n_rows, n_selected, kind, mode)
            got = twice(lambda narrow: gpu_ctx.assoc_resident(token, row_map, X_src.shape[1], case.col_map, masks,
                                                              narrow_hash=narrow, **flags_of(mode)), what)
            same(got, expected(V, tbits, mode), what)
    assert turn >= 100


def run_dev(ctx, X, col_map, tbits, mode, what, pad_ones=False):
    """pgx_assoc_dev on caller memory (tests/dev_entry_checks.py): results and a workspace of exactly the size asked for,
    between guard bands, full of either garbage pattern, on a side stream whose earlier work makes the inputs; without and
    with the narrow hash. An empty column map is handed over as a NULL pointer. Returns the result dict."""
    import dev_entry_checks as chk
    from pangenomix_amd import _native
    n_rows, n_genomes = X.shape
    n_selected = n_genomes if col_map is None else int(col_map.size)
    n_targets = tbits.shape[0]
    masks = es.pack_masks(tbits, pad_ones)
    bits = es.bitmap(X, _native.lib().pgx_bitmap_stride_words(n_rows))
    nws = _native.lib().pgx_assoc_workspace_bytes(n_rows, n_selected)
    assert nws > 0
    results = []
    for fill in chk.FILLS:
        runs = []
        with chk.stream_scope('side') as st:
            inputs = [chk.upload(bits)] + [chk.upload(a) if a is not None and a.size else None for a in (col_map, masks)]
            u_bits, u_map, u_masks = inputs
            with chk.unchanged(*[u for u in inputs if u is not None]):
                for narrow in (False, True):
                    ws, tp = chk.guarded(nws, fill), chk.guarded(n_targets * n_rows * 4, fill) if n_targets else None
                    inc, block, rep = (chk.guarded(n_rows * 4, fill) for _ in range(3))
                    nb = ctx.assoc_dev(u_bits.ptr, n_rows, n_genomes, u_map.ptr if u_map else None, n_selected,
                                       u_masks.ptr if u_masks else None, n_targets, tp.ptr if tp else None, inc.ptr, block.ptr,
                                       rep.ptr, ws.ptr, nws, stream=st, narrow_hash=narrow, **flags_of(mode))
                    runs.append((nb, ws, tp, inc, block, rep))
        for nb, ws, tp, inc, block, rep in runs:
            for b in (ws, tp, inc, block, rep):
                if b is not None:
                    b.assert_guards_intact()
            got = {'incidence': inc.numpy(np.uint32),
                   'tp': tp.numpy(np.uint32).reshape(n_targets, n_rows) if tp else np.zeros((0, n_rows), dtype=np.uint32),
                   'block_of_row': None, 'rep_row': None}
            if mode == 'no_blocks':                          # only tp and incidence are written
                assert nb == 0 and block.is_still_garbage() and rep.is_still_garbage(), what
            else:
                assert 0 <= nb <= n_rows, what
                got['block_of_row'], got['rep_row'] = block.numpy(np.int32), rep.numpy(np.int32)[:nb]
                assert (rep.numpy(np.uint8)[nb * 4:] == fill).all(), (what, 'rep_row was written behind n_blocks')
            results.append(got)
    for other in results[1:]:
        same_bytes(results[0], other, (what, 'garbage pattern or narrow hash'))
    return results[0]


@pytest.mark.parametrize('n_rows', es.N_ROWS)
def test_sweep_device_entry(n_rows, gpu_ctx):
    """assoc_dev: at every n_selected one case of the sweep -- which one moves on with n_rows and n_selected, so that the
    twelve row counts together take every generator and selection through this entry -- in one flag setting and with 0, 1
    or 3 masks in turn."""
    at = es.N_ROWS.index(n_rows)
    for i, n_selected in enumerate(es.N_SELECTED):
        cases = list(es.cases(n_rows, n_selected))
        turn = at * len(es.N_SELECTED) + i
        case = cases[(5 * at + i) % len(cases)]
        mode, n_targets = MODES[turn % 3], N_TARGETS[(turn // 3) % 3]
        tbits = es.target_bits(es.rng_for(7, n_rows, n_selected), n_targets, n_selected)
        what = (case.name, n_rows, n_selected, mode, n_targets)
        got = run_dev(gpu_ctx, case.X, case.col_map, tbits, mode, what)
        same(got, expected(es.view(case.X, case.col_map), tbits, mode), what)


def test_the_device_entry_sweep_takes_every_generator_and_selection():
    """(needs no device: the choice made in test_sweep_device_entry, counted)"""
    names, kinds, settings = set(), set(), set()
    for at, n_rows in enumerate(es.N_ROWS):
        for i, n_selected in enumerate(es.N_SELECTED):
            cases = list(es.cases(n_rows, n_selected))
            turn = at * len(es.N_SELECTED) + i
            name, kind = cases[(5 * at + i) % len(cases)].name.split('/')
            names.add(name)
            kinds.add(kind)
            settings.add((MODES[turn % 3], N_TARGETS[(turn // 3) % 3]))
    assert names == set(es.GENERATORS) and kinds == set(es.SELECTIONS) and len(settings) == 9


def test_the_bitmap_of_the_edge_sets_is_the_device_s(gpu_ctx):
    from pangenomix_amd import _native
    X = es.empty_rows_at_the_edges(es.rng_for(1), 1025, 70, None)
    r, c = coo(X)
    assert np.array_equal(gpu_ctx.presence_bitmap(r, c, 1025, 70), es.bitmap(X, _native.lib().pgx_bitmap_stride_words(1025)))


# ---------------------------------------------------------------------------------------------------------------------
# the block table under pressure (narrow hash: chains as long as there are blocks, wrapping at the end of the table)

PRESSURE = [('all_distinct', 32, 70, None),        # cap = 64 = 2 n_rows: exactly half full, the chain wraps
            ('all_distinct', 33, 70, None),        # cap = 128
            ('all_distinct', 2049, 70, None),      # a chain of 2049 slots, two words to compare
            ('all_equal', 5000, 130, None),        # every row takes the same chain; atomicMin under full contention
            ('few_patterns', 4097, 200, 40)]       # 40 blocks of about 100 rows each


@pytest.mark.parametrize('name,n_rows,n_genomes,k', PRESSURE, ids=['%s_%d' % (p[0], p[1]) for p in PRESSURE])
def test_block_table_under_pressure(name, n_rows, n_genomes, k, gpu_ctx):
    """Blocks and drop-empty blocks with the narrow hash equal the model and the plain run; three narrow-hash calls give
    the same bytes (which row owns a slot differs from run to run, the outputs must not)."""
    rng = es.rng_for(8, n_rows)
    X = es.GENERATORS[name](rng, n_rows, n_genomes, None, **({'k': k} if k else {}))
    r, c = coo(X)
    tbits = es.target_bits(rng, 1, n_genomes)
    masks = es.pack_masks(tbits)
    for mode in ('blocks', 'drop_empty'):
        what = (name, n_rows, mode)
        call = lambda narrow: gpu_ctx.assoc(r, c, n_rows, n_genomes, None, masks, narrow_hash=narrow, **flags_of(mode))[0]  # noqa: E731
        got = twice(call, what)
        same(got, expected(X, tbits, mode), what)
        for _ in range(2):
            same_bytes(call(True), got, (what, 'run to run'))
    if name == 'all_distinct':
        assert np.array_equal(got['rep_row'], np.arange(n_rows))


# ---------------------------------------------------------------------------------------------------------------------
# the rounds of the prefix scan (1024 flag words = 65536 rows per round), without the flag

@pytest.mark.parametrize('n_rows', (65535, 65536, 65537))
def test_prefix_scan_rounds_all_rows_distinct(n_rows, gpu_ctx):
    """flag_words = 1024, 1024, 1025: one full round, then a second round of a single word."""
    X = es.all_distinct(es.rng_for(9, n_rows), n_rows, 17, None)
    got = gpu_ctx.assoc(*coo(X), n_rows, 17, blocks=True)[0]
    assert np.array_equal(got['block_of_row'], np.arange(n_rows)) and np.array_equal(got['rep_row'], np.arange(n_rows))
    same(got, expected(X, np.zeros((0, 17), dtype=bool), 'blocks'), n_rows)


def test_prefix_scan_every_first_row_in_the_second_round(gpu_ctx):
    """65536 empty rows, then 300 rows of 9 patterns: with drop_empty every block's first row lies in the second round of
    the scan (flag words 1024..1028) and the whole first round counts nothing; without it the empty rows are block 0."""
    n_rows = 65536 + 300
    rng = es.rng_for(10)
    X = np.zeros((n_rows, 70), dtype=bool)
    tail = es.few_patterns(rng, 300, 70, None, k=9)
    tail[:, 0] |= ~tail.any(axis=1)
    X[65536:] = tail
    none = np.zeros((0, 70), dtype=bool)
    for mode in ('drop_empty', 'blocks'):
        got = gpu_ctx.assoc(*coo(X), n_rows, 70, **flags_of(mode))[0]
        same(got, expected(X, none, mode), mode)
        assert got['rep_row'][-9:].min() >= 65536 and got['rep_row'].size == (9 if mode == 'drop_empty' else 10)


# ---------------------------------------------------------------------------------------------------------------------
# contracts of include/pgx.h

@pytest.mark.parametrize('n_selected', (0, 1, 63, 65, 127, 129, 193))
def test_mask_pad_bits_are_ignored(n_selected, gpu_ctx):
    """Masks with every pad bit set give the tp of masks with them clear, and both the model's: host entry, resident
    entry and device entry."""
    rng = es.rng_for(11, n_selected)
    n_rows = 257
    n_genomes, col_map = es.selection('prefix' if n_selected else 'empty', n_selected, rng)
    X = rng.random((n_rows, n_genomes)) < 0.5
    V, (r, c) = es.view(X, col_map), coo(X)
    tbits = es.target_bits(rng, 3, n_selected)
    tbits[0] = True                                         # (a mask that is all ones up to the pad bits, then beyond)
    want = expected(V, tbits, 'no_blocks')
    clear, ones = es.pack_masks(tbits), es.pack_masks(tbits, pad_ones=True)
    assert (clear != ones).any()
    token = make_resident(gpu_ctx, X)
    for masks in (clear, ones):
        same(gpu_ctx.assoc(r, c, n_rows, n_genomes, col_map, masks)[0], want, n_selected)
        same(gpu_ctx.assoc_resident(token, np.arange(n_rows), n_genomes, col_map, masks), want, n_selected)
    same(run_dev(gpu_ctx, X, col_map, tbits, 'no_blocks', n_selected, pad_ones=True), want, n_selected)


@pytest.mark.parametrize('n_rows', (1, 64, 257))
def test_empty_selection(n_rows, gpu_ctx):
    """n_selected = 0 of 16 genomes: incidence and tp are 0, all rows form one block, under drop_empty no row is in a block.
    The device entry gets a NULL column map for it. A NULL map with any other n_selected != n_genomes stays refused."""
    from pangenomix_amd import _native
    rng = es.rng_for(12, n_rows)
    n_genomes, col_map = es.selection('empty', 0, rng)
    X = rng.random((n_rows, n_genomes)) < 0.5
    r, c = coo(X)
    tbits = np.zeros((3, 0), dtype=bool)
    masks = es.pack_masks(tbits, pad_ones=True)
    token = make_resident(gpu_ctx, X)
    for mode in MODES:
        want = expected(X[:, :0], tbits, mode)
        assert not want['incidence'].any() and not want['tp'].any() and want['tp'].shape == (3, n_rows)
        if mode == 'blocks':
            assert not want['block_of_row'].any() and list(want['rep_row']) == [0]
        if mode == 'drop_empty':
            assert (want['block_of_row'] == -1).all() and want['rep_row'].size == 0
        what = ('empty selection', n_rows, mode)
        same(twice(lambda narrow: gpu_ctx.assoc(r, c, n_rows, n_genomes, col_map, masks, narrow_hash=narrow,
                                                **flags_of(mode))[0], what), want, what)
        same(twice(lambda narrow: gpu_ctx.assoc_resident(token, np.arange(n_rows), n_genomes, col_map, masks,
                                                         narrow_hash=narrow, **flags_of(mode)), what), want, what)
        same(run_dev(gpu_ctx, X, col_map, tbits, mode, what, pad_ones=True), want, what)
    import torch
    d = torch.zeros(4096, dtype=torch.int32, device='cuda')
    nws = _native.lib().pgx_assoc_workspace_bytes(8, 5)
    assert 0 < nws <= d.numel() * 4
    torch.cuda.synchronize()
    with pytest.raises(_native.PgxError, match='without a column map every genome is selected'):
        gpu_ctx.assoc_dev(d.data_ptr(), 8, n_genomes, None, 5, None, 0, None, d.data_ptr(), d.data_ptr(), d.data_ptr(),
                          d.data_ptr(), nws)


def test_repeated_genomes_count_once_per_column(gpu_ctx):
    """A col_map that names one genome three times: each of its columns counts in incidence and tp, and the blocks are
    those of the table with the repeated columns (the model's X[:, col_map])."""
    rng = es.rng_for(13)
    n_genomes, col_map = es.selection('repeats', 65, rng)
    X = es.few_patterns(rng, 257, n_genomes, col_map, k=7)
    X[:, col_map[0]] = rng.random(257) < 0.5
    tbits = np.ones((1, 65), dtype=bool)
    V = es.view(X, col_map)
    got = twice(lambda narrow: gpu_ctx.assoc(*coo(X), 257, n_genomes, col_map, es.pack_masks(tbits), blocks=True,
                                             narrow_hash=narrow)[0], 'repeats')
    same(got, expected(V, tbits, 'blocks'), 'repeats')
    once = X[:, np.unique(col_map)].sum(axis=1)                                # every selected genome counted once
    assert np.array_equal(got['incidence'], once + 2 * X[:, col_map[0]])
    assert np.array_equal(got['tp'][0], got['incidence'])
