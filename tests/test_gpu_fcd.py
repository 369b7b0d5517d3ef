"""Formal concept decomposition on the device (pangenomix_amd/fcd.py, csrc/fcd.hip) against the reference's results
(tests/golden/fcd) and, where no fixture exists, against the numpy model of the same rule (tests/fcd_model.py, itself
checked against every fixture in tests/test_fcd_host.py). Every comparison is exact."""
import glob
import os

import numpy as np
import pytest
import scipy.sparse

import fcd_model
from pangenomix_amd import fcd, sparse_utils, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, 'tests', 'golden', 'fcd', '*.npz')))
NAMES = [os.path.basename(p)[:-4] for p in FIXTURES]


def same_concepts(got, want, kind):
    assert len(got) == len(want)
    box = tuple if kind == 'tuple' else list
    for (gx, gy), (wx, wy) in zip(got, want):
        assert type(gx) is box and type(gy) is box
        assert list(gx) == list(wx) and list(gy) == list(wy)


def check_factorisation(S, W, H, F, overlap):
    S = np.asarray(S) != 0
    assert W.dtype == np.dtype(int) and H.dtype == np.dtype(int)
    assert W.shape == (S.shape[0], len(F)) and H.shape == (len(F), S.shape[1])
    P = W @ H
    if overlap:
        assert np.array_equal(P > 0, S)
    else:
        assert np.array_equal(P, S.astype(int))


@pytest.mark.parametrize('path', FIXTURES, ids=NAMES)
def test_every_fixture_exactly(path, gpu_ctx):
    fx = fcd_model.load_fixture(path)
    S = fx['dense']()
    np.random.seed(12345)
    W, H, F = fcd.formal_concept_decomposition(S, ctx=gpu_ctx, **fx['kwargs'])
    st = np.random.get_state()
    same_concepts(F, fx['F'], fx['kind'])
    assert st[2] == fx['pos'] and np.array_equal(st[1], fx['key'])
    W2, H2 = fcd.decompose_from_concepts(S, F)
    assert np.array_equal(W, W2) and np.array_equal(H, H2)
    if fx['kwargs']['limit'] is None:                     # a complete decomposition factors the table
        check_factorisation(S, W, H, F, fx['kwargs']['overlap'])
    if fx['coverage'] is not None:
        cov = fcd.compute_concept_coverage(S, F, log_rate=0, ctx=gpu_ctx)
        assert cov.dtype == np.float64 and np.array_equal(cov, fx['coverage'])
        assert cov[-1] == 1.0


def test_dense_sparse_and_lsdf_inputs_agree(gpu_ctx):
    fx = fcd_model.load_fixture(os.path.join(ROOT, 'tests', 'golden', 'fcd', 'blocks_1500x90_overlap.npz'))
    S = fx['dense']()
    coo = scipy.sparse.coo_matrix((np.ones(fx['rows'].size, dtype=np.int64), (fx['rows'], fx['cols'])), shape=fx['shape'])
    perm = np.random.default_rng(5).permutation(coo.nnz)               # coordinates in no particular order
    scrambled = scipy.sparse.coo_matrix((coo.data[perm], (coo.row[perm], coo.col[perm])), shape=fx['shape'])
    lsdf = sparse_utils.LightSparseDataFrame(['r%d' % i for i in range(fx['shape'][0])],
                                             ['c%d' % j for j in range(fx['shape'][1])], coo)
    for kw in ({}, {'overlap': True}, {'dim_balance': True}, {'seed': 5, 'limit': 30}):
        results = [fcd.formal_concept_decomposition(X, ctx=gpu_ctx, **kw)
                   for X in (S, S.astype(bool), S.astype(np.float32), coo.tocsr(), scrambled, lsdf)]
        for W, H, F in results[1:]:
            assert F == results[0][2] and np.array_equal(W, results[0][0]) and np.array_equal(H, results[0][1])
    cov = [fcd.compute_concept_coverage(X, fx['F'], log_rate=0, ctx=gpu_ctx) for X in (S, coo.tocsr(), lsdf)]
    assert np.array_equal(cov[0], fx['coverage']) and np.array_equal(cov[1], cov[0]) and np.array_equal(cov[2], cov[0])


def test_duplicate_coordinates_are_refused(gpu_ctx):
    dup = scipy.sparse.coo_matrix((np.ones(3, dtype=np.int64), ([0, 1, 0], [0, 1, 0])), shape=(2, 2))
    with pytest.raises(ValueError, match='duplicate'):
        fcd.formal_concept_decomposition(dup, ctx=gpu_ctx)
    with pytest.raises(ValueError, match='duplicate'):
        fcd.compute_concept_coverage(dup, [((0,), (0,))], ctx=gpu_ctx)
    with pytest.raises(ValueError, match='twice'):
        fcd.compute_concept_coverage(np.eye(3), [((0, 0), (0,))], ctx=gpu_ctx)
    with pytest.raises(IndexError):
        fcd.compute_concept_coverage(np.eye(3), [((3,), (0,))], ctx=gpu_ctx)


def test_seed_with_overlap_reads_the_shuffled_table(gpu_ctx):
    """The one deliberate deviation: the reference mixes the table before and after the shuffle there."""
    fx = fcd_model.load_fixture(os.path.join(ROOT, 'tests', 'golden', 'fcd', 'blocks_1500x90_overlap.npz'))
    S = fx['dense']()
    W, H, F = fcd.formal_concept_decomposition(S, overlap=True, seed=3, ctx=gpu_ctx)
    state = np.random.get_state()
    want = fcd_model.formal_concepts(S, overlap=True, seed=3)
    same_concepts(F, want, 'list')
    assert state[2] == np.random.get_state()[2] and np.array_equal(state[1], np.random.get_state()[1])
    check_factorisation(S, W, H, F, True)


def test_large_table_equals_the_model(gpu_ctx):
    r, c, G = synth.pancore_matrix(20000, 200, 3)
    S = np.zeros((G, 200), dtype=bool)
    S[r, c] = True
    coo = scipy.sparse.coo_matrix((np.ones(r.size, dtype=np.int64), (r, c)), shape=(G, 200))
    for kw in ({'limit': 60}, {'limit': 25, 'dim_balance': True}, {'limit': 12, 'overlap': True}):
        F = fcd.formal_concept_decomposition(coo, sort_components=False, ctx=gpu_ctx, **kw)[2]
        assert F == fcd_model.decompose(S, **kw)
        assert len(F) == kw['limit']


def test_resident_bitmap_path_equals_the_upload_path(tmp_path, gpu_ctx):
    """The gene table build_cds_pangenome() returns is decomposed from the bitmap the pipeline left on the device (rows =
    cluster numbers, gathered into the decomposition's own working copy): same result as uploading the coordinates, the
    resident bitmap is not modified, and estimate_pan_core_size() on the same object is unchanged afterwards."""
    from pangenomix_amd import _native, pangenome
    from pangenomix_amd import pangenome_analysis as pa
    ctx = _native.default_context()
    paths = synth.ProteinSet(9, 300, 400, 90, 5).write_faa(str(tmp_path / 'g'))
    (tmp_path / 'o').mkdir()
    _, dfg = pangenome.build_cds_pangenome(paths, str(tmp_path / 'o'), name='R')
    res = dfg._pgx_resident
    G, S = dfg.shape
    before = ctx.bitmap_resident_read(res['token'], G, S)
    plain = sparse_utils.LightSparseDataFrame(list(dfg.index), list(dfg.columns), dfg.data.copy())     # no hand-off
    assert fcd._table(dfg)[3] is res and fcd._table(plain)[3] is None
    np.random.seed(3)
    curves = pa.estimate_pan_core_size(plain, 20)
    for kw in ({}, {'overlap': True}, {'dim_balance': True, 'sort_components': False}, {'seed': 4}, {'limit': 5}):
        a = fcd.formal_concept_decomposition(dfg, ctx=ctx, **kw)
        b = fcd.formal_concept_decomposition(plain, ctx=ctx, **kw)
        assert a[2] == b[2] and len(a[2]) > 0 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert a[2] == fcd_model.formal_concepts(dfg.values, **kw)
    check_factorisation(dfg.values, *fcd.formal_concept_decomposition(dfg, ctx=ctx), overlap=False)
    assert np.array_equal(ctx.bitmap_resident_read(res['token'], G, S), before)
    np.random.seed(3)
    assert pa.estimate_pan_core_size(dfg, 20).equals(curves)


def test_two_calls_in_a_row_reuse_the_workspace(gpu_ctx):
    import torch
    fx = fcd_model.load_fixture(os.path.join(ROOT, 'tests', 'golden', 'fcd', 'blocks_3000x120.npz'))
    S = fx['dense']()
    first = fcd.formal_concept_decomposition(S, ctx=gpu_ctx)[2]
    fcd.compute_concept_coverage(S, first, log_rate=0, ctx=gpu_ctx)
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info()[0]
    for _ in range(2):
        assert fcd.formal_concept_decomposition(S, ctx=gpu_ctx)[2] == first
        fcd.compute_concept_coverage(S, first, log_rate=0, ctx=gpu_ctx)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free_before


def test_device_pointer_entry(gpu_ctx):
    """pgx_fcd_dev on a bitmap and a workspace of the caller (torch tensors) equals the host entry; the bitmap is not written."""
    import torch
    from pangenomix_amd import _native
    fx = fcd_model.load_fixture(os.path.join(ROOT, 'tests', 'golden', 'fcd', 'rows_193.npz'))
    n_rows, n_cols = fx['shape']
    bits = gpu_ctx.presence_bitmap(fx['rows'], fx['cols'], n_rows, n_cols)
    d_bits = torch.from_numpy(bits.view(np.int64)).cuda()
    nws = _native.lib().pgx_fcd_workspace_bytes(n_rows, n_cols)
    d_ws = torch.empty(nws, dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    for kw in ({}, {'overlap': True}, {'dim_factors': fcd._dim_factors(n_rows, n_cols)}):
        got = gpu_ctx.fcd_dev(d_bits.data_ptr(), n_rows, n_cols, n_rows * n_cols, d_ws.data_ptr(), nws, **kw)
        want, dup = gpu_ctx.fcd(fx['rows'], fx['cols'], n_rows, n_cols, n_rows * n_cols, **kw)
        assert dup == 0 and got['ones_left'] == 0 and got['ones_total'] == fx['rows'].size
        for k in ('rows', 'row_offsets', 'cols', 'col_offsets', 'left'):
            assert np.array_equal(got[k], want[k])
    assert np.array_equal(d_bits.cpu().numpy().view(np.uint64), bits)
    with pytest.raises(_native.PgxError, match='workspace too small'):
        gpu_ctx.fcd_dev(d_bits.data_ptr(), n_rows, n_cols, 1, d_ws.data_ptr(), nws - 1)
    # the same with a workspace of exactly that size between guard bands and full of garbage, on a side stream whose
    # earlier work makes the bitmap (tests/dev_entry_checks.py)
    import dev_entry_checks as chk
    want = gpu_ctx.fcd(fx['rows'], fx['cols'], n_rows, n_cols, n_rows * n_cols)[0]
    for fill in chk.FILLS:
        with chk.stream_scope('side') as st:
            ws = chk.guarded(nws, fill)
            up = chk.upload(bits)
            with chk.unchanged(up):
                got = gpu_ctx.fcd_dev(up.ptr, n_rows, n_cols, n_rows * n_cols, ws.ptr, nws, stream=st)
        ws.assert_guards_intact()
        for k in ('rows', 'row_offsets', 'cols', 'col_offsets', 'left'):
            assert np.array_equal(got[k], want[k])


def test_verbose_prints_the_progress_line(capsys, gpu_ctx):
    fx = fcd_model.load_fixture(os.path.join(ROOT, 'tests', 'golden', 'fcd', 'duplicate_rows.npz'))
    S = fx['dense']()
    fcd.formal_concept_decomposition(S, verbose=True, ctx=gpu_ctx)
    lines = capsys.readouterr().out.strip().split('\n')
    cov = fcd_model.coverage(S, fcd_model.decompose(S))
    assert lines == ['Components found: %d | Coverage: %s' % (i, cov[i]) for i in range(1, len(cov))]


@pytest.mark.slow
def test_full_benchmark_table_is_factored(gpu_ctx):
    r, c, G = synth.pancore_matrix(150000, 400, 1)
    coo = scipy.sparse.coo_matrix((np.ones(r.size, dtype=np.int64), (r, c)), shape=(G, 400))
    F, shape, info = fcd._concepts(coo, ctx=gpu_ctx)
    assert info['ones_left'] == 0 and info['ones_total'] == r.size
    assert sum(len(x) * len(y) for x, y in F) == r.size              # every one covered exactly once ...
    covered = np.zeros(shape, dtype=bool)
    for x, y in F:
        covered[np.ix_(x, y)] = True
    assert covered.sum() == r.size and covered[r, c].all()            # ... and no zero covered
    cov = fcd.compute_concept_coverage(coo, F, log_rate=0, ctx=gpu_ctx)
    assert cov[-1] == 1.0 and np.all(np.diff(cov) > 0)
