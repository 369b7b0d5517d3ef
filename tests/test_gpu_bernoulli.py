"""compute_bernoulli_grid_core_genome on the GPU against fixtures produced by the reference itself (tests/golden/core,
tests/golden/make_golden_core.py).

Tolerances: an evaluation's LL within rtol 1e-12 and each gradient entry within 1e-12 x the sum of the absolute values
of its terms (the device sums in another order, and takes log p + log q for present cells when every p q is a normal
number below 1); nan and inf exactly where the reference has them; the whole call's optimum LL within rtol 1e-10 and every P
and Q within atol 1e-7, with nit, nfev and status equal. (Relative noise of 1e-13 on the reference's LL and gradient
moves its optimum by at most 4e-14 in LL and 5e-10 in P and Q at 2,000 x 400 and 8,000 x 400, nit and nfev unchanged.)

The LL rtol 1e-12 holds on these fixtures because their absent cells make |LL| large. It is not what the kernel promises
on every table: log(fl(p q)) carries up to 2^-53 of absolute error per present cell, the fast mode's log p + log q does
not, and on a table without absent cells near the upper bound |log(p q)| is only about 1e-8 per cell. There the two
forms differ by far more than 1e-12 relatively (in numpy, 128 x 12 table of ones: 1.3e-11 with P, Q in [0.9999999,
0.99999999], 5.5e-10 with everything at 0.99999999), the fast mode being the accurate one against 50 digits. The
bound that holds everywhere is 1e-12 x (sum of LL's absolute terms) + 2^-52 x (present cells): tests/bernoulli_model.py,
applied in tests/test_gpu_bernoulli_edges.py and tests/test_gpu_bernoulli_geometry.py."""
import contextlib
import glob
import io
import os

import numpy as np
import pandas as pd
import pytest
import scipy.optimize
import scipy.sparse

from pangenomix_amd import _native, pangenome, sparse_utils, synth
from pangenomix_amd import pangenome_analysis as pa

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = sorted(p for p in glob.glob(os.path.join(HERE, 'golden', 'core', '*.npz'))
               if not p.endswith('to_sparse_arrays.npz'))
IDS = [os.path.basename(p)[:-4] for p in CASES]


def dense_frame(z):
    G, S = (int(v) for v in z['shape'])
    X = np.zeros((G, S), dtype=np.int64)
    X[z['rows'], z['cols']] = 1
    return pd.DataFrame(X, index=list(z['index']), columns=list(z['columns']))


def lsdf(z):
    G, S = (int(v) for v in z['shape'])
    m = scipy.sparse.coo_matrix((np.ones(z['rows'].size, dtype=np.int64), (z['rows'], z['cols'])), shape=(G, S))
    return sparse_utils.LightSparseDataFrame(list(z['index']), list(z['columns']), m)


def call_args(z):
    freqs = z['init_gene_freqs']
    return dict(prob_bounds=tuple(z['prob_bounds']), init_capture_prob=float(z['init_capture_prob']),
                init_gene_freqs=None if freqs.size == 0 else freqs)


def assert_same_specials(got, want):
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_array_equal(np.isposinf(got), np.isposinf(want))
    np.testing.assert_array_equal(np.isneginf(got), np.isneginf(want))


def assert_evaluation(out, ll, grad, scale):
    assert_same_specials(out[:1], np.array([ll]))
    if np.isfinite(ll):
        np.testing.assert_allclose(out[0], ll, rtol=1e-12, atol=0)
    assert_same_specials(out[1:], grad)
    fin = np.isfinite(grad)
    err = np.abs(out[1:][fin] - grad[fin])
    assert np.all(err <= 1e-12 * scale[fin]), err.max()


@pytest.mark.parametrize('path', CASES, ids=IDS)
def test_evaluations_match_the_reference(path, gpu_ctx):
    z = np.load(path)
    G, S = (int(v) for v in z['shape'])
    assert gpu_ctx.bernoulli_load(z['rows'], z['cols'], G, S) == 0
    for k, pt in enumerate(z['points']):
        for exact in (False, True):
            out = gpu_ctx.bernoulli_eval(pt, exact=exact)
            assert_evaluation(out, z['point_ll'][k], z['point_grad'][k], z['point_scale'][k])
            again = gpu_ctx.bernoulli_eval(pt, exact=exact)
            assert out.tobytes() == again.tobytes()                  # bit-identical from call to call
    # pan/core calls on the same context build ANOTHER table (another shape) through the same upload helper, in slots
    # of their own: the loaded table is still the one that is evaluated
    before = gpu_ctx.bernoulli_eval(z['points'][0])
    rng = np.random.default_rng(5)
    G2, S2 = G + 70, S + 3
    r2, c2 = (a.astype(np.int32) for a in np.nonzero(rng.random((G2, S2)) < 0.5))
    perms = np.array([rng.permutation(S2) for _ in range(3)], dtype=np.int32)
    pan, core, dup = gpu_ctx.pan_core_coo(r2, c2, G2, S2, perms)
    counts, dup2 = gpu_ctx.row_counts(r2, c2, G2, S2)
    assert dup == 0 and dup2 == 0 and pan[0, -1] == np.count_nonzero(counts) and int(counts.sum()) == r2.size
    assert gpu_ctx.bernoulli_eval(z['points'][0]).tobytes() == before.tobytes()


def test_pad_bits_are_not_cells(gpu_ctx):
    """An empty table of 65 genes (63 pad bits in its last word): every gene and genome term is an absent cell's."""
    G, S = 65, 3
    assert gpu_ctx.bernoulli_load(np.zeros(0, np.int32), np.zeros(0, np.int32), G, S) == 0
    P, Q = np.full(G, 0.9), np.full(S, 0.95)
    out = gpu_ctx.bernoulli_eval(np.concatenate((P, Q)))
    t = 1.0 - 0.9 * 0.95
    np.testing.assert_allclose(out[0], G * S * np.log(t), rtol=1e-13)
    np.testing.assert_allclose(out[1:G + 1], -S * 0.95 / t, rtol=1e-13)
    np.testing.assert_allclose(out[G + 1:], -G * 0.9 / t, rtol=1e-13)


@pytest.mark.parametrize('path', CASES, ids=IDS)
def test_whole_call_matches_the_reference(path, gpu_ctx):
    z = np.load(path)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        df_opt, res = pa.compute_bernoulli_grid_core_genome(dense_frame(z), ctx=gpu_ctx, **call_args(z))
    assert list(df_opt.index) == list(z['labels']) and list(df_opt.columns) == ['initial', 'optimum']
    init, opt = df_opt['initial'].values, df_opt['optimum'].values
    assert_same_specials(init, z['initial'])
    fin = np.isfinite(z['initial'])
    np.testing.assert_allclose(init[fin], z['initial'][fin], rtol=1e-12, atol=0)
    assert (res.nit, res.nfev, res.status) == (int(z['nit']), int(z['nfev']), int(z['status']))
    assert_same_specials(opt[:1], z['optimum'][:1])
    if np.isfinite(z['optimum'][0]):
        np.testing.assert_allclose(opt[0], z['optimum'][0], rtol=1e-10)
    np.testing.assert_allclose(opt[1:], z['optimum'][1:], rtol=0, atol=1e-7)
    np.testing.assert_allclose(res.x, z['x'], rtol=0, atol=1e-7)
    lines = [ln for ln in buf.getvalue().splitlines() if ln.startswith(('Initial loglikelihood:', 'Final loglikelihood:'))]
    want = [ln for ln in z['printed'] if ln.startswith(('Initial loglikelihood:', 'Final loglikelihood:'))]
    assert [ln.split(':')[0] for ln in lines] == [ln.split(':')[0] for ln in want]
    for a, b in zip(lines, want):
        va, vb = float(a.split(':')[1]), float(b.split(':')[1])
        assert (np.isnan(va) and np.isnan(vb)) or np.isclose(va, vb, rtol=1e-10, atol=0)


def test_input_forms_give_identical_results(gpu_ctx):
    """Dense frame, LightSparseDataFrame and to_sparse_arrays() frame: the same bits."""
    z = np.load([p for p in CASES if 'g128' in p][0])
    results = []
    for table in (dense_frame(z), lsdf(z), lsdf(z).to_sparse_arrays()):
        with contextlib.redirect_stdout(io.StringIO()):
            df_opt, res = pa.compute_bernoulli_grid_core_genome(table, ctx=gpu_ctx)
        results.append((df_opt, res))
    for df_opt, res in results[1:]:
        assert df_opt.equals(results[0][0])
        assert res.x.tobytes() == results[0][1].x.tobytes() and (res.nit, res.nfev) == (results[0][1].nit, results[0][1].nfev)


def test_resident_pipeline_table(tmp_path, monkeypatch):
    """build_cds_pangenome()'s gene table is evaluated from the bitmap the pipeline left on the device (rows = cluster
    numbers, which the names order as strings: C10 before C2), with no upload; it agrees with the uploaded table within
    the evaluation tolerance. A later pipeline makes the token stale and the call uploads the coordinates instead. The
    Heaps fit in between must not disturb the resident bitmap."""
    ctx = _native.default_context()
    paths = synth.ProteinSet(9, 300, 400, 90, 5).write_faa(str(tmp_path / 'g1'))
    (tmp_path / 'o1').mkdir()
    with contextlib.redirect_stdout(io.StringIO()):
        dfa, dfg = pangenome.build_cds_pangenome(paths, str(tmp_path / 'o1'), name='B')
    G, S = dfg.shape
    row_cluster = dfg._pgx_resident['row_cluster']
    assert G >= 11 and not np.array_equal(row_cluster, np.arange(G))
    np.testing.assert_array_equal(row_cluster, [int(str(x).rsplit('_C', 1)[1]) for x in dfg.index])
    plain = sparse_utils.LightSparseDataFrame(list(dfg.index), list(dfg.columns), dfg.data.copy())
    np.random.seed(1)
    with contextlib.redirect_stdout(io.StringIO()):
        pa.fit_heaps_by_iteration(pa.estimate_pan_core_size(dfg, 20), ctx=ctx)
    uploads = []
    real_load = _native.Context.bernoulli_load
    monkeypatch.setattr(_native.Context, 'bernoulli_load', lambda self, *a: uploads.append(1) or real_load(self, *a))
    with contextlib.redirect_stdout(io.StringIO()):
        a_opt, a_res = pa.compute_bernoulli_grid_core_genome(dfg)
    assert uploads == []
    with contextlib.redirect_stdout(io.StringIO()):
        b_opt, b_res = pa.compute_bernoulli_grid_core_genome(plain)
    assert uploads == [1]
    # evaluation tolerance at the start point and at the uploaded call's optimum
    coo = plain.data.tocoo()
    X = np.zeros((G, S))
    X[coo.row, coo.col] = 1
    for pt in (b_opt['initial'].values[1:], b_res.x):
        ctx.bernoulli_load(coo.row, coo.col, G, S)
        want = ctx.bernoulli_eval(pt)
        ctx.bernoulli_load_resident(dfg._pgx_resident['token'], row_cluster, S)
        got = ctx.bernoulli_eval(pt)
        P, Q = pt[:G], pt[G:]
        t = 1.0 - np.outer(P, Q)
        scale = np.concatenate((X.sum(1) / P + ((1 - X) * Q / t).sum(1), X.sum(0) / Q + ((1 - X) * P[:, None] / t).sum(0)))
        np.testing.assert_allclose(got[0], want[0], rtol=1e-12)
        assert np.all(np.abs(got[1:] - want[1:]) <= 1e-12 * scale)
    del uploads[:]                                            # (the loads just above)
    np.testing.assert_allclose(a_opt['optimum'].values[0], b_opt['optimum'].values[0], rtol=1e-10)
    np.testing.assert_allclose(a_res.x, b_res.x, rtol=0, atol=1e-7)
    assert (a_res.nit, a_res.nfev, a_res.status) == (b_res.nit, b_res.nfev, b_res.status)
    # a later pipeline replaces the resident bitmap: the call falls back to the upload
    paths2 = synth.ProteinSet(5, 200, 300, 60, 6).write_faa(str(tmp_path / 'g2'))
    (tmp_path / 'o2').mkdir()
    with contextlib.redirect_stdout(io.StringIO()):
        pangenome.build_cds_pangenome(paths2, str(tmp_path / 'o2'), name='B2')
    with pytest.raises(_native.PgxError):
        ctx.bernoulli_load_resident(dfg._pgx_resident['token'], row_cluster, S)
    with contextlib.redirect_stdout(io.StringIO()):
        c_opt, c_res = pa.compute_bernoulli_grid_core_genome(dfg)
    assert uploads == [1]
    assert c_opt.equals(b_opt) and c_res.x.tobytes() == b_res.x.tobytes()


@pytest.mark.slow
def test_full_size_against_a_numpy_restatement(gpu_ctx):
    """40,000 x 400: the device-driven call against the same scipy call driven by the model's likelihood and gradient
    written out in numpy here."""
    rng = np.random.default_rng(11)
    G, S = 40000, 400
    p = rng.uniform(0.6, 1.0, G)
    q = rng.uniform(0.97, 1.0, S)
    X = rng.random((G, S)) < np.outer(p, q)
    rows, cols = np.nonzero(X)
    m = scipy.sparse.coo_matrix((np.ones(rows.size, dtype=np.int64), (rows, cols)), shape=(G, S))
    table = sparse_utils.LightSparseDataFrame(['g%d' % i for i in range(G)], ['s%d' % j for j in range(S)], m)
    with contextlib.redirect_stdout(io.StringIO()):
        df_opt, res = pa.compute_bernoulli_grid_core_genome(table, ctx=gpu_ctx)

    Xf = X.astype(np.float64)
    absent = 1.0 - Xf
    rowsum, colsum = Xf.sum(1), Xf.sum(0)

    def negative(pq):
        P, Q = pq[:G], pq[G:]
        r = np.outer(P, Q)
        t = 1.0 - r
        ll = (Xf * np.log(r)).sum() + (absent * np.log(t)).sum()
        w = absent / t
        grad = np.concatenate((rowsum / P - w @ Q, colsum / Q - P @ w))
        return -ll, -grad

    x0 = np.clip(np.concatenate((rowsum / float(S), 0.9999 * np.ones(S))), 0.8, 0.99999999)
    want = scipy.optimize.minimize(negative, x0, method='L-BFGS-B', jac=True, bounds=[(0.8, 0.99999999)] * (G + S))
    np.testing.assert_allclose(df_opt['initial'].values[0], -negative(x0)[0], rtol=1e-12)
    np.testing.assert_allclose(-res.fun, -want.fun, rtol=1e-10)
    np.testing.assert_allclose(res.x, want.x, rtol=0, atol=1e-7)
    assert (res.nit, res.nfev, res.status) == (want.nit, want.nfev, want.status)
