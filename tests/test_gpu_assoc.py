"""The association screen on the device (pangenomix_amd/ml_pipelines.py, sparse_utils.compress_rows*, csrc/assoc.hip)
against the reference's results (tests/golden/assoc) and, where no fixture exists, against the numpy model of the same
rules (tests/assoc_model.py, itself checked against every fixture in tests/test_assoc_host.py). Every comparison is exact
except the LOR (assoc_checks.LOR_ATOL)."""
import contextlib
import glob
import io
import os

import numpy as np
import pandas as pd
import pytest
import scipy.sparse

import assoc_checks
import assoc_model
from pangenomix_amd import ml_pipelines, sparse_utils, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'assoc')
TABLES = sorted(glob.glob(os.path.join(GOLDEN, 'table_*.npz')))
PREPARE = sorted(glob.glob(os.path.join(GOLDEN, 'prepare_*.npz')))
PREFILTER = sorted(glob.glob(os.path.join(GOLDEN, 'prefilter_*.npz')))
ids = lambda paths: [os.path.basename(p)[:-4] for p in paths]      # noqa: E731


def quiet(fn, *args, **kwargs):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*args, **kwargs)


def coo_of(r, c, shape):
    return scipy.sparse.coo_matrix((np.ones(r.size, dtype=np.int64), (r, c)), shape=shape)


def labelled(coo):
    return sparse_utils.LightSparseDataFrame(np.array(['g%d' % i for i in range(coo.shape[0])]),
                                             np.array(['s%d' % j for j in range(coo.shape[1])]), coo)


def resident_frame(ctx, r, c, shape, rng):
    """An LSDF as build_cds_pangenome() hands it over: its bitmap is left on the device by bitmap_from_clusters (one
    record per entry, rows = cluster numbers) and row i of the frame is cluster perm[i]."""
    G, S = shape
    token = ctx.bitmap_from_clusters(r, np.arange(r.size), c.astype(np.uint32), np.arange(S), G, S)
    perm = rng.permutation(G)
    inv = np.empty(G, dtype=np.int64)
    inv[perm] = np.arange(G)
    lsdf = labelled(coo_of(inv[r], c, shape))
    lsdf._pgx_resident = {'ctx': ctx, 'token': token, 'shape': lsdf.shape, 'data': lsdf.data, 'nnz': int(lsdf.data.nnz),
                          'row_cluster': perm.astype(np.int32)}
    return lsdf


@pytest.mark.parametrize('path', TABLES, ids=ids(TABLES))
def test_every_table_fixture(path, gpu_ctx):
    fx = assoc_model.load_table_fixture(path)
    assoc_checks.check_blocks(fx, gpu_ctx)
    assoc_checks.check_contingency(fx, gpu_ctx)


@pytest.mark.parametrize('path', PREPARE, ids=ids(PREPARE))
def test_prepare_fixtures_upload_and_resident(path, gpu_ctx):
    assoc_checks.check_prepare(path, gpu_ctx)
    d = np.load(path)
    own = assoc_checks.prepare_inputs(d)[0]
    own._pgx_resident = {'ctx': gpu_ctx, 'shape': own.shape, 'data': own.data, 'nnz': int(own.data.nnz),
                         'row_cluster': np.arange(own.shape[0], dtype=np.int32),
                         'token': gpu_ctx.bitmap_from_clusters(own.data.row, np.arange(own.data.nnz), own.data.col.astype(np.uint32),
                                                               np.arange(own.shape[1]), own.shape[0], own.shape[1])}
    assoc_checks.check_prepare(path, gpu_ctx, own)


@pytest.mark.parametrize('path', PREFILTER, ids=ids(PREFILTER))
def test_prefilter_fixtures(path, gpu_ctx):
    assoc_checks.check_prefilter(path, gpu_ctx)


def test_two_dimensional_target_equals_the_stacked_calls(gpu_ctx):
    rng = np.random.default_rng(4)
    r, c, G = synth.pancore_matrix(20000, 200, 3)
    coo = coo_of(r, c, (G, 200))
    targets = (rng.random((32, 200)) < rng.random((32, 1))).astype(float)
    targets[3, rng.random(200) < 0.3] = np.nan
    targets[4] *= rng.random(200) * 2.5
    both = ml_pipelines.contingency_tables_from_sparse(coo, targets, ctx=gpu_ctx)
    assert both.shape == (32, G, 4)
    X = assoc_model.dense(r, c, (G, 200))
    for t in range(32):
        one = ml_pipelines.contingency_tables_from_sparse(coo, targets[t], ctx=gpu_ctx)
        assert np.array_equal(one, both[t], equal_nan=True)
        assert np.array_equal(one, assoc_model.contingency(X, targets[t]), equal_nan=True)


def test_every_input_container_gives_the_same(gpu_ctx):
    fx = assoc_model.load_table_fixture(os.path.join(GOLDEN, 'table_samples_400_duplicates.npz'))
    X = assoc_model.dense(fx['rows'], fx['cols'], fx['shape'])
    coo = assoc_checks.fixture_matrix(fx)
    perm = np.random.default_rng(5).permutation(coo.nnz)
    scrambled = scipy.sparse.coo_matrix((coo.data[perm], (coo.row[perm], coo.col[perm])), shape=coo.shape)
    for S in (X.astype(np.int64), X, X.astype(np.float32), coo.tocsr(), scrambled, labelled(coo)):
        assoc_checks.check_blocks(fx, gpu_ctx, S)
        assoc_checks.check_contingency(fx, gpu_ctx, S)


def test_duplicates_and_stored_zeros_are_refused(gpu_ctx):
    dup = scipy.sparse.coo_matrix((np.ones(3, dtype=np.int64), ([0, 1, 0], [0, 1, 0])), shape=(2, 2))
    zero = scipy.sparse.coo_matrix((np.array([1, 0]), ([0, 1], [0, 1])), shape=(2, 2))
    for bad, match in ((dup, 'duplicate'), (zero, 'stored zeros')):
        with pytest.raises(ValueError, match=match):
            sparse_utils.compress_rows_spmatrix(bad, ctx=gpu_ctx)
        with pytest.raises(ValueError, match=match):
            ml_pipelines.contingency_tables_from_sparse(bad, np.ones(2), ctx=gpu_ctx)


def same_table(frame, X):
    """frame (an LSDF) holds the bool table X (compared sparse: the benchmark's tables are not densified as int64)."""
    return frame.shape == X.shape and (frame.data.tocsr().astype(bool) != scipy.sparse.csr_matrix(X)).nnz == 0


def check_against_model(ctx, lsdf, X, rng, n_drugs=2):
    """Blocks, contingency and the whole per-drug screen of the table X (held by lsdf) against assoc_model: without a
    column selection and with one that keeps about half the genomes."""
    G, S = X.shape
    block_of_row, rep_row = assoc_model.blocks(X)
    lsdf_block, defs = sparse_utils.compress_rows(lsdf, ctx=ctx)
    assert lsdf_block.shape == (rep_row.size, S) and len(defs) == rep_row.size
    assert same_table(lsdf_block, X[rep_row])
    members = np.concatenate(defs)
    sizes = np.array([len(x) for x in defs])
    assert np.array_equal(members, lsdf.index[np.argsort(block_of_row, kind='stable')])
    assert np.array_equal(sizes, np.bincount(block_of_row))
    y = (rng.random(S) < 0.3).astype(float)
    assert np.array_equal(ml_pipelines.contingency_tables_from_sparse(lsdf, y, ctx=ctx), assoc_model.contingency(X, y))
    pheno = (rng.random((S, n_drugs)) < 0.4).astype(float)
    pheno[rng.random((S, n_drugs)) < 0.5] = np.nan
    drugs = ['drug%d' % k for k in range(n_drugs)]
    df_amr = pd.DataFrame(pheno, index=lsdf.columns, columns=drugs)
    df_known = pd.DataFrame(np.full((3, n_drugs), 1.0), index=lsdf.index[:3], columns=drugs)
    for k, drug in enumerate(drugs):
        genomes, kept, b, rep, selected = assoc_model.screen(X, pheno[:, k], min_freq=3, max_features=2000)
        amr, known, feat, block, cdefs = quiet(ml_pipelines.prepare_amr_case_data, drug, lsdf, df_amr, df_known, ctx=ctx)
        assert list(amr.index) == list(lsdf.columns[genomes]) and known == set(lsdf.index[:3])
        assert list(feat.index) == list(lsdf.index[kept]) and list(feat.columns) == list(lsdf.columns[genomes])
        assert same_table(feat, X[kept][:, genomes])
        assert same_table(block, X[kept][rep][:, genomes])
        assert np.array_equal(np.concatenate(cdefs), lsdf.index[kept][np.argsort(b, kind='stable')])
        assert np.array_equal(np.array([len(x) for x in cdefs]), np.bincount(b))
        assert selected.size == 2000                    # (the case reaches the LOR selection)
        got = quiet(ml_pipelines.prefilter_features_by_lor, block, amr, min_freq=3, max_features=2000, ctx=ctx)
        assert list(got.index) == ['B%d' % i for i in selected]


def test_333_x_1000_against_the_model(gpu_ctx):
    rng = np.random.default_rng(12)
    X = (rng.random((24, 1000)) < 0.05)[rng.integers(0, 24, 333)]
    X[rng.random(333) < 0.5, 977] ^= True                   # rows that differ in one late column only
    r, c = np.nonzero(X)
    for lsdf in (labelled(coo_of(r, c, X.shape)), resident_frame(gpu_ctx, r, c, X.shape, rng)):
        Xl = lsdf.values != 0
        block_of_row, rep_row = assoc_model.blocks(Xl)
        spblock, defs = sparse_utils.compress_rows_spmatrix(lsdf, ctx=gpu_ctx)
        assert [[int(v) for v in x] for x in defs] == assoc_model.definitions(block_of_row, rep_row.size)
        assert np.array_equal(spblock.toarray() != 0, Xl[rep_row])
        targets = (rng.random((5, 1000)) < 0.5).astype(float)
        got = ml_pipelines.contingency_tables_from_sparse(lsdf, targets, ctx=gpu_ctx)
        for t in range(5):
            assert np.array_equal(got[t], assoc_model.contingency(Xl, targets[t]))
        pheno = np.where(rng.random(1000) < 0.5, np.nan, (rng.random(1000) < 0.4).astype(float))
        df_amr = pd.DataFrame({'d': pheno}, index=lsdf.columns)
        df_known = pd.DataFrame({'d': [1.0]}, index=lsdf.index[:1])
        genomes, kept, b, rep, _ = assoc_model.screen(Xl, pheno)
        _, _, feat, block, cdefs = quiet(ml_pipelines.prepare_amr_case_data, 'd', lsdf, df_amr, df_known, ctx=gpu_ctx)
        assert list(feat.index) == list(lsdf.index[kept]) and np.array_equal(block.values != 0, Xl[kept][rep][:, genomes])
        assert [list(x) for x in cdefs] == [list(lsdf.index[kept][np.asarray(m, dtype=np.int64)])
                                            for m in assoc_model.definitions(b, rep.size)]


def test_benchmark_table_against_the_model_upload_and_resident(gpu_ctx):
    """pancore_matrix() (150,000 x 400): blocks, contingency and two drugs' screens, from uploaded coordinates and from
    the resident bitmap (rows permuted against it); the resident bitmap is not written: estimate_pan_core_size() on the
    same object returns what it returned before."""
    from pangenomix_amd import pangenome_analysis as pa
    rng = np.random.default_rng(2)
    r, c, G = synth.pancore_matrix(150000, 400, 1)
    plain = labelled(coo_of(r, c, (G, 400)))
    check_against_model(gpu_ctx, plain, assoc_model.dense(r, c, (G, 400)), rng)
    res = resident_frame(gpu_ctx, r, c, (G, 400), rng)
    assert sparse_utils._screen_table(res, 'test')[3] is res._pgx_resident
    before = gpu_ctx.bitmap_resident_read(res._pgx_resident['token'], G, 400)
    np.random.seed(3)
    curves = quiet(pa.estimate_pan_core_size, res, 10, ctx=gpu_ctx)
    check_against_model(gpu_ctx, res, assoc_model.dense(res.data.row, res.data.col, res.shape), rng)
    assert np.array_equal(gpu_ctx.bitmap_resident_read(res._pgx_resident['token'], G, 400), before)
    np.random.seed(3)
    assert quiet(pa.estimate_pan_core_size, res, 10, ctx=gpu_ctx).equals(curves)


def test_blocks_are_the_same_on_every_run(gpu_ctx):
    r, c, G = synth.pancore_matrix(150000, 400, 1)
    first = gpu_ctx.assoc(r, c, G, 400, blocks=True)[0]
    assert first['rep_row'].size > 100000
    for _ in range(2):
        again = gpu_ctx.assoc(r, c, G, 400, blocks=True)[0]
        for k in ('block_of_row', 'rep_row', 'incidence'):
            assert np.array_equal(again[k], first[k])


def test_all_rows_distinct_and_all_rows_equal(gpu_ctx):
    n = 70000
    X = ((np.arange(1, n + 1)[:, None] >> np.arange(17)[None, :]) & 1).astype(bool)
    out = gpu_ctx.assoc(*np.nonzero(X), n, 17, blocks=True)[0]
    assert np.array_equal(out['block_of_row'], np.arange(n)) and np.array_equal(out['rep_row'], np.arange(n))
    X = np.tile(np.random.default_rng(1).random(130) < 0.5, (n, 1))
    out = gpu_ctx.assoc(*np.nonzero(X), n, 130, blocks=True)[0]
    assert not out['block_of_row'].any() and list(out['rep_row']) == [0]
    spblock, defs = sparse_utils.compress_rows_spmatrix(X[:5000], ctx=gpu_ctx)
    assert spblock.shape == (1, 130) and [int(v) for v in defs[0]] == list(range(5000))


def test_prefilter_selection_path_against_the_model(gpu_ctx):
    rng = np.random.default_rng(8)
    X, y = assoc_checks.tie_table(rng)
    for min_freq, max_features in ((0, 7), (0, 100), (3, 50)):
        assoc_checks.check_selection_against_model(X, y, min_freq, max_features, gpu_ctx)
    assoc_checks.check_selection_against_model(X, np.zeros(40), 0, 10, gpu_ctx)          # every LOR is NaN


def test_device_pointer_entry_and_errors(gpu_ctx):
    """pgx_assoc_dev on a bitmap, maps, masks, results and a workspace of the caller (torch tensors) equals the host
    entry; the bitmap is not written; a column map entry out of range is an error, not a read."""
    import torch
    from pangenomix_amd import _native
    fx = assoc_model.load_table_fixture(os.path.join(GOLDEN, 'table_samples_400.npz'))
    n_rows, n_cols = fx['shape']
    rng = np.random.default_rng(3)
    col_map = rng.permutation(n_cols)[:170].astype(np.int32)
    masks = ml_pipelines._target_masks((rng.random((3, 170)) < 0.5).astype(float))
    want = gpu_ctx.assoc(fx['rows'], fx['cols'], n_rows, n_cols, col_map, masks, blocks=True, drop_empty=True)[0]
    X = assoc_model.dense(fx['rows'], fx['cols'], fx['shape'])[:, col_map]
    assert np.array_equal(want['incidence'], X.sum(axis=1)) and np.array_equal(want['block_of_row'] < 0, ~X.any(axis=1))
    bits = gpu_ctx.presence_bitmap(fx['rows'], fx['cols'], n_rows, n_cols)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()                   # noqa: E731
    d_bits, d_map, d_masks = dev(bits.view(np.int64)), dev(col_map), dev(masks.view(np.int64))
    nws = _native.lib().pgx_assoc_workspace_bytes(n_rows, 170)
    d_ws = torch.empty(nws, dtype=torch.uint8, device='cuda')
    d_tp = torch.empty((3, n_rows), dtype=torch.int32, device='cuda')
    d_inc, d_block, d_rep = (torch.empty(n_rows, dtype=torch.int32, device='cuda') for _ in range(3))
    torch.cuda.synchronize()
    args = (d_bits.data_ptr(), n_rows, n_cols, d_map.data_ptr(), 170, d_masks.data_ptr(), 3, d_tp.data_ptr(),
            d_inc.data_ptr(), d_block.data_ptr(), d_rep.data_ptr(), d_ws.data_ptr())
    n_blocks = gpu_ctx.assoc_dev(*args, nws, blocks=True, drop_empty=True)
    assert n_blocks == want['rep_row'].size
    assert np.array_equal(d_tp.cpu().numpy().view(np.uint32), want['tp'])
    assert np.array_equal(d_inc.cpu().numpy().view(np.uint32), want['incidence'])
    assert np.array_equal(d_block.cpu().numpy(), want['block_of_row'])
    assert np.array_equal(d_rep.cpu().numpy()[:n_blocks], want['rep_row'])
    assert np.array_equal(d_bits.cpu().numpy().view(np.uint64), bits)
    with pytest.raises(_native.PgxError, match='workspace too small'):
        gpu_ctx.assoc_dev(*args, nws - 1)
    bad = col_map.copy()
    bad[5] = n_cols
    with pytest.raises(_native.PgxError, match='out of range'):
        gpu_ctx.assoc(fx['rows'], fx['cols'], n_rows, n_cols, bad, masks)
    d_bad = dev(bad)
    with pytest.raises(_native.PgxError, match='out of range'):
        gpu_ctx.assoc_dev(args[0], n_rows, n_cols, d_bad.data_ptr(), *args[4:], nws)
    # the same with results and a workspace of exactly that size between guard bands and full of garbage, on a side
    # stream whose earlier work makes the inputs (tests/dev_entry_checks.py)
    import dev_entry_checks as chk
    results = []
    for fill in chk.FILLS:
        with chk.stream_scope('side') as st:
            ws, tp = chk.guarded(nws, fill), chk.guarded(3 * n_rows * 4, fill)
            inc, block, rep = (chk.guarded(n_rows * 4, fill) for _ in range(3))
            u_bits, u_map, u_masks = chk.upload(bits), chk.upload(col_map), chk.upload(masks)
            with chk.unchanged(u_bits, u_map, u_masks):
                nb = gpu_ctx.assoc_dev(u_bits.ptr, n_rows, n_cols, u_map.ptr, 170, u_masks.ptr, 3, tp.ptr, inc.ptr, block.ptr,
                                       rep.ptr, ws.ptr, nws, blocks=True, drop_empty=True, stream=st)
        for b in (ws, tp, inc, block, rep):
            b.assert_guards_intact()
        assert nb == want['rep_row'].size
        results.append((tp.numpy(np.uint32).reshape(3, n_rows), inc.numpy(np.uint32), block.numpy(np.int32),
                        rep.numpy(np.int32)[:nb]))
    got = chk.same_bytes(results)
    for g, k in zip(got, ('tp', 'incidence', 'block_of_row', 'rep_row')):
        assert np.array_equal(g, want[k])


def test_calls_in_a_row_reuse_the_workspace(gpu_ctx):
    import torch
    fx = assoc_model.load_table_fixture(os.path.join(GOLDEN, 'table_samples_400_duplicates.npz'))
    coo = assoc_checks.fixture_matrix(fx)
    sparse_utils.compress_rows_spmatrix(coo, ctx=gpu_ctx)
    ml_pipelines.contingency_tables_from_sparse(coo, fx['targets'], ctx=gpu_ctx)
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info()[0]
    for _ in range(2):
        sparse_utils.compress_rows_spmatrix(coo, ctx=gpu_ctx)
        ml_pipelines.contingency_tables_from_sparse(coo, fx['targets'], ctx=gpu_ctx)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free_before


# -- the host entries' transfers ---------------------------------------------------------------------------------------
def pack_targets(targets):
    """uint64 [n_targets, words] of bool [n_targets, n_selected]: bit j & 63 of word j >> 6 = selected genome j"""
    targets = np.asarray(targets, dtype=bool)
    words = max(1, (targets.shape[1] + 63) // 64)
    bits = np.zeros((targets.shape[0], words * 64), dtype=bool)
    bits[:, :targets.shape[1]] = targets
    return np.packbits(bits, axis=1, bitorder='little').view('<u8').astype(np.uint64).reshape(targets.shape[0], words)


def small_table(n_genomes):
    """Seven rows of which only four can differ (so n_blocks < n_rows), the two empty ones among them."""
    rng = np.random.default_rng(n_genomes)
    base = rng.random((3, n_genomes)) < 0.5
    base[:, 0], base[0, -1], base[1, -1] = True, True, False
    X = np.vstack([base[[0, 1, 0, 2, 1]], np.zeros((2, n_genomes), dtype=bool)])[[5, 0, 1, 2, 6, 3, 4]]
    return X


@pytest.mark.parametrize('n_genomes', (3, 70))
def test_small_tables_through_both_host_entries(n_genomes, gpu_ctx):
    rng = np.random.default_rng(100 + n_genomes)
    X = small_table(n_genomes)
    n_rows = X.shape[0]
    r, c = (a.astype(np.int32) for a in np.nonzero(X))
    token = gpu_ctx.bitmap_from_clusters(r, np.arange(r.size), c.astype(np.uint32), np.arange(n_genomes), n_rows, n_genomes)
    perm = rng.permutation(n_rows).astype(np.int32)
    col_map = rng.permutation(n_genomes)[:max(2, n_genomes // 2)].astype(np.int32)
    for cmap in (None, col_map):
        for name, table, call in (('upload', X, lambda **kw: gpu_ctx.assoc(r, c, n_rows, n_genomes, **kw)[0]),
                                  ('resident', X[perm], lambda **kw: gpu_ctx.assoc_resident(token, perm, n_genomes, **kw))):
            sub = table if cmap is None else table[:, cmap]
            targets = rng.random((2, sub.shape[1])) < 0.5
            block_of_row, rep_row = assoc_model.blocks(sub)
            assert rep_row.size < n_rows
            for masks, blocks in ((None, False), (None, True), (targets, False), (targets, True)):
                out = call(col_map=cmap, masks=None if masks is None else pack_targets(masks), blocks=blocks)
                what = (name, cmap is not None, masks is not None, blocks)
                assert np.array_equal(out['incidence'], sub.sum(axis=1)), what
                if masks is None:
                    assert out['tp'].shape == (0, n_rows), what
                else:
                    assert np.array_equal(out['tp'], (sub[None, :, :] & masks[:, None, :]).sum(axis=2)), what
                if blocks:
                    assert np.array_equal(out['block_of_row'], block_of_row) and np.array_equal(out['rep_row'], rep_row), what
                else:
                    assert out['block_of_row'] is None and out['rep_row'] is None, what


def test_host_entry_leaves_rep_row_behind_n_blocks_as_the_caller_had_it(gpu_ctx):
    import ctypes as C
    from pangenomix_amd import _native
    lib, P, h = _native.lib(), _native._ptr, gpu_ctx._h
    X = small_table(3)
    n_rows = X.shape[0]
    block_of_row, rep_row = assoc_model.blocks(X)
    r, c = (a.astype(np.int32) for a in np.nonzero(X))
    sentinel = 0x5C5C5C5C
    inc = np.full(n_rows, sentinel, dtype=np.uint32)
    block, rep = np.full(n_rows, sentinel, dtype=np.int32), np.full(n_rows, sentinel, dtype=np.int32)
    n_blocks, dup = C.c_uint32(77), C.c_uint64(77)
    rc = lib.pgx_assoc(h, P(r), P(c), r.size, n_rows, 3, None, 3, None, 0, _native.ASSOC_BLOCKS, None, P(inc), P(block), P(rep),
                       C.byref(n_blocks), C.byref(dup))
    assert rc == 0 and dup.value == 0 and n_blocks.value == rep_row.size < n_rows
    assert np.array_equal(inc, X.sum(axis=1)) and np.array_equal(block, block_of_row)
    assert np.array_equal(rep[:rep_row.size], rep_row)
    assert (rep[rep_row.size:] == sentinel).all(), 'rep_row was written behind n_blocks'
