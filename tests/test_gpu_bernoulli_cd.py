"""compute_bernoulli_grid_core_genome_cd on the GPU against fixtures produced by the reference itself
(tests/golden/bernoulli_cd, tests/golden/make_golden_bernoulli_cd.py) and against the numpy model
(tests/bernoulli_cd_model.py).

Tolerances. P and Q of every iteration: bernoulli_cd_model.TOL = 2 (xtol + rtol) = 4.1e-12 -- two points
that each satisfy Brent's stopping rule for the same root lie that close when the noise of f is negligible; the model
itself stays within a tenth of that of every fixture (tests/test_bernoulli_cd_host.py; measured 1.2e-16), so no
fixture needs a wider one. LL (row 0): against the per-cell numpy likelihood AT THE DEVICE'S OWN solver variables under
DESIGN.md 6a's rule, 1e-12 x (sum of absolute terms) + 2^-52 x (present cells), and against the fixture's LL within
sum_k |dLL/dx_k| x TOL plus that bound. The recorder's conditions (a) and (b) keep every boundary decision of the
fixtures out of reach of the order of summation, so the boundary rule is compared bit for bit."""
import contextlib
import io

import numpy as np
import pytest
import torch

import bernoulli_cd_model as model
import dev_entry_checks as chk
import test_bernoulli_cd_host as host
from pangenomix_amd import _native, pangenome, sparse_utils, synth
from pangenomix_amd import pangenome_analysis as pa

pytestmark = pytest.mark.gpu
LOGS = _native.BERNOULLI_CD_LOGS


def entry(table, ctx, **kwargs):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        df = pa.compute_bernoulli_grid_core_genome_cd(table, ctx=ctx, **kwargs)
    return df, buf.getvalue()


def assert_ll_at_own_variables(X, table, solver, use_logs):
    for k in range(table.shape[1]):
        ll, scale, present = model.likelihood(X, solver[1:, k], use_logs)
        bound = model.ll_bound(scale, present)
        print('column %d: |LL - per-cell sum at the solver variables| %.3g (bound %.3g)' % (k, abs(table[0, k] - ll), bound))
        assert abs(table[0, k] - ll) <= bound
        assert solver[0, k] == table[0, k]


# ---- 1. every fixture, both flavours, through the Python entry ---------------------------------------------------------
@pytest.mark.parametrize('path', host.FIXTURES, ids=host.IDS)
def test_entry_matches_the_reference(path, gpu_ctx):
    z = np.load(path)
    args = host.call_args(z)
    df, printed = entry(host.dense_frame(z), gpu_ctx, **args)
    assert list(df.index) == list(z['labels']) and list(df.columns) == list(range(args['n_iterations'] + 1))
    table = df.values
    assert np.all(np.isfinite(table))
    host.assert_table_matches_the_fixture(table, z, model.TOL)
    host.assert_printed_matches_the_fixture(printed, table, z)
    # the solver's own variables of the same call (the table is still loaded): same bits, and LL is their per-cell sum
    lo, hi = args['prob_bounds']
    again, solver = gpu_ctx.bernoulli_cd(host.start_point(z), args['init_capture_prob'], lo, hi, args['n_iterations'],
                                         use_logs=args['use_logs'], solver_table=True)
    assert again.tobytes() == table.tobytes()
    X = model.dense(z['rows'], z['cols'], z['shape'])
    assert_ll_at_own_variables(X, table, solver, args['use_logs'])
    if args['use_logs']:
        np.testing.assert_allclose(table[1:], np.exp(solver[1:]), rtol=4 * 2.0 ** -52, atol=0)
    else:
        assert solver.tobytes() == table.tobytes()
    stats = gpu_ctx.bernoulli_cd_stats()
    n_solves = args['n_iterations'] * (table.shape[0] - 1)
    assert stats['not_converged'] == 0 and stats['solves'] == n_solves
    assert 2 * n_solves <= stats['evaluations'] and stats['max_evaluations'] <= 2 + model.MAXITER


# ---- 2. the boundary rule in isolation --------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['g128_s64', 'g129_s65', 'g4100_s5', 'g5_s300', 'g70_s9_freqs', 'g70_s9_bounds', 'g1_s1'])
@pytest.mark.parametrize('use_logs', [False, True])
def test_boundary_rule_gives_the_fixtures_bounds_bit_for_bit(name, use_logs, gpu_ctx):
    """The row of ones (gene 1), the row of zeros (gene 2) or the column of ones (genome 1) of each table, and every
    other solve that took the boundary branch in the reference: the value is lo or hi itself, the one the fixture has.
    Plain flavour: the table's bits are the bound's. Log flavour: the solver's variable is bit for bit the library's
    log lo or log hi (one value each in the whole table, within one ulp of numpy's), the side is the fixture's, and the
    table holds its exp."""
    z = host.fixture(name + ('_logs' if use_logs else ''))
    args = host.call_args(z)
    lo, hi = args['prob_bounds']
    X = model.dense(z['rows'], z['cols'], z['shape'])
    G, S = X.shape
    gpu_ctx.bernoulli_load(z['rows'], z['cols'], G, S)
    table, solver = gpu_ctx.bernoulli_cd(host.start_point(z), args['init_capture_prob'], lo, hi, args['n_iterations'],
                                         use_logs=use_logs, solver_table=True)
    special = [1 + i for i in range(G) if X[i].all() or not X[i].any()] + [1 + G + j for j in range(S) if X[:, j].all()]
    assert special
    on_bound = np.zeros(table.shape, dtype=bool)
    on_bound[1:, 1:] = z['boundary'].T
    assert all(on_bound[r, 1:].all() for r in special)
    want = z['table'][on_bound]
    want_hi = np.abs(want - hi) < np.abs(want - lo)
    if not use_logs:
        assert set(np.unique(want)) <= {lo, hi}
        assert table[on_bound].tobytes() == want.tobytes()
    else:
        got = solver[on_bound]
        los, his = np.unique(got[~want_hi]), np.unique(got[want_hi])
        assert los.size <= 1 and his.size <= 1
        for v, ref in ((los, np.log(lo)), (his, np.log(hi))):
            assert v.size == 0 or abs(v[0] - ref) <= np.spacing(abs(ref))
        np.testing.assert_allclose(table[on_bound], want, rtol=4 * 2.0 ** -52, atol=0)
    # no other solve sits on a bound by the rule: the interior ones are strictly inside
    inside = ~on_bound
    inside[0, :] = False
    inside[:, 0] = False
    blo, bhi = (np.log(lo), np.log(hi)) if use_logs else (lo, hi)
    assert np.all((solver[inside] >= blo - np.spacing(abs(blo))) & (solver[inside] <= bhi + np.spacing(abs(bhi))))


# ---- 3. the same bits on a second call and from every input form -------------------------------------------------------
@pytest.mark.parametrize('use_logs', [False, True])
def test_input_forms_and_second_calls_give_identical_bits(use_logs, gpu_ctx):
    z = host.fixture('g128_s64' + ('_logs' if use_logs else ''))
    args = host.call_args(z)
    frames = [host.dense_frame(z), host.dense_frame(z), host.lsdf(z), host.lsdf(z).to_sparse_arrays()]
    tables = [entry(f, gpu_ctx, **args)[0] for f in frames]
    for t in tables[1:]:
        assert t.values.tobytes() == tables[0].values.tobytes() and t.equals(tables[0])


def test_resident_pipeline_table_gives_the_uploaded_tables_bits(tmp_path, monkeypatch):
    """build_cds_pangenome()'s gene table runs from the bitmap the pipeline left on the device, with no upload."""
    ctx = _native.default_context()
    paths = synth.ProteinSet(9, 300, 400, 90, 5).write_faa(str(tmp_path / 'g1'))
    (tmp_path / 'o1').mkdir()
    with contextlib.redirect_stdout(io.StringIO()):
        dfa, dfg = pangenome.build_cds_pangenome(paths, str(tmp_path / 'o1'), name='B')
    plain = sparse_utils.LightSparseDataFrame(list(dfg.index), list(dfg.columns), dfg.data.copy())
    uploads = []
    real_load = _native.Context.bernoulli_load
    monkeypatch.setattr(_native.Context, 'bernoulli_load', lambda self, *a: uploads.append(1) or real_load(self, *a))
    for use_logs in (False, True):
        del uploads[:]
        a = entry(dfg, None, n_iterations=2, prob_bounds=(0.05, 0.999), use_logs=use_logs)[0]
        assert uploads == []
        b = entry(plain, None, n_iterations=2, prob_bounds=(0.05, 0.999), use_logs=use_logs)[0]
        assert uploads == [1]
        assert a.values.tobytes() == b.values.tobytes() and a.equals(b)
        assert ctx.bernoulli_cd_stats()['not_converged'] == 0


# ---- 4. Context.bernoulli_cd_dev on caller tensors and streams ---------------------------------------------------------
def stride_words(n_rows):
    return int(_native.lib().pgx_bitmap_stride_words(int(n_rows)))


def bitmap(X, pad_ones=False):
    """genome-major, gene g = bit g & 63 of word g >> 6 (pgx.h); pad_ones: every bit beyond n_genes set"""
    G, S = X.shape
    stride = stride_words(G)
    dense = np.full((S, stride * 64), bool(pad_ones))
    dense[:, :G] = X.T
    return np.packbits(dense, axis=1, bitorder='little').view('<u8').astype(np.uint64)


def cd_ws_bytes(G, S):
    return int(_native.lib().pgx_bernoulli_cd_workspace_bytes(G, S))


def run_dev(ctx, kind, fill, bits, G, S, init_p, init_q, lo, hi, T, flags, with_solver=True):
    nws = cd_ws_bytes(G, S)
    cells = (1 + G + S) * (T + 1)
    with chk.stream_scope(kind) as st:
        table, ws = chk.guarded(cells * 8, fill), chk.guarded(nws, fill)
        solver = chk.guarded(cells * 8, fill) if with_solver else None
        d_bits, d_p = chk.upload(bits), chk.upload(init_p)
        with chk.unchanged(d_bits, d_p):
            ctx.bernoulli_cd_dev(d_bits.ptr, G, S, d_p.ptr, init_q, lo, hi, T, table.ptr, solver.ptr if solver else None,
                                 ws.ptr, nws, flags, st)
    table.assert_guards_intact(), ws.assert_guards_intact()
    out = (table.numpy(np.float64).reshape(1 + G + S, T + 1),)
    if solver:
        solver.assert_guards_intact()
        out += (solver.numpy(np.float64).reshape(1 + G + S, T + 1),)
    return out


@pytest.mark.parametrize('name', ['g65_s63', 'g129_s65_logs', 'g70_s9_iter0', 'g1_s1_logs'])
def test_bernoulli_cd_dev_on_caller_tensors_and_streams(name, gpu_ctx):
    """Garbage in the results and the workspace (two patterns: the same bytes), guard bands intact, inputs unchanged,
    stream 0 and a busy side stream, pad bits set in the caller's bitmap beyond n_genes: the host entry's bits."""
    z = host.fixture(name)
    args = host.call_args(z)
    lo, hi = args['prob_bounds']
    flags = LOGS if args['use_logs'] else 0
    X = model.dense(z['rows'], z['cols'], z['shape'])
    G, S = X.shape
    p0, T = host.start_point(z), args['n_iterations']
    gpu_ctx.bernoulli_load(z['rows'], z['cols'], G, S)
    want = gpu_ctx.bernoulli_cd(p0, args['init_capture_prob'], lo, hi, T, use_logs=args['use_logs'], solver_table=True)
    host.assert_table_matches_the_fixture(want[0], z, model.TOL)
    for kind in chk.STREAMS:
        for pad_ones in (False, True):
            got = chk.same_bytes([run_dev(gpu_ctx, kind, f, bitmap(X, pad_ones), G, S, p0, args['init_capture_prob'],
                                          lo, hi, T, flags) for f in chk.FILLS])
            assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    only, = run_dev(gpu_ctx, 'null', 0xFF, bitmap(X), G, S, p0, args['init_capture_prob'], lo, hi, T, flags,
                    with_solver=False)
    assert only.tobytes() == want[0].tobytes()


def test_bernoulli_cd_dev_does_not_allocate(gpu_ctx):
    z = host.fixture('g64_s7')
    X = model.dense(z['rows'], z['cols'], z['shape'])
    G, S = X.shape
    nws = cd_ws_bytes(G, S)
    d_bits, d_p = chk.upload(bitmap(X)), chk.upload(host.start_point(z))
    table, ws = chk.guarded((1 + G + S) * 4 * 8, 0xFF), chk.guarded(nws, 0xFF)
    chk.assert_no_allocation(lambda: gpu_ctx.bernoulli_cd_dev(d_bits.ptr, G, S, d_p.ptr, 0.9999, 0.8, 0.99999999, 3,
                                                              table.ptr, None, ws.ptr, nws, 0, 0))
    host.assert_table_matches_the_fixture(table.numpy(np.float64).reshape(1 + G + S, 4), z, model.TOL)


# ---- 5. every refusal; n_iterations = 0 -----------------------------------------------------------------------------------
REFUSALS = [
    dict(lo=0.0), dict(lo=-0.5), dict(lo=0.9, hi=0.9), dict(lo=0.95, hi=0.9), dict(hi=1.0), dict(hi=1.5),
    dict(lo=np.nan), dict(hi=np.nan), dict(hi=np.inf), dict(init_q=0.0), dict(init_q=-1.0), dict(init_q=np.nan),
    dict(init_q=np.inf), dict(init_q=1.00000002), dict(flags=2), dict(flags=3), dict(G=0), dict(S=0), dict(T=2 ** 20 + 1),
]


@pytest.mark.parametrize('bad', REFUSALS, ids=[','.join('%s=%r' % kv for kv in r.items()) for r in REFUSALS])
def test_refusals_leave_the_outputs_untouched(bad, gpu_ctx):
    z = host.fixture('g64_s7')
    X = model.dense(z['rows'], z['cols'], z['shape'])
    a = dict(G=X.shape[0], S=X.shape[1], lo=0.8, hi=0.99999999, init_q=0.9999, T=3, flags=0)
    a.update(bad)
    nws = cd_ws_bytes(*X.shape)
    d_bits, d_p = chk.upload(bitmap(X)), chk.upload(host.start_point(z))
    table, solver, ws = (chk.guarded((1 + sum(X.shape)) * 4 * 8, 0x5A), chk.guarded((1 + sum(X.shape)) * 4 * 8, 0x5A),
                         chk.guarded(nws, 0x5A))
    with pytest.raises(_native.PgxError) as err:
        gpu_ctx.bernoulli_cd_dev(d_bits.ptr, a['G'], a['S'], d_p.ptr, a['init_q'], a['lo'], a['hi'], a['T'], table.ptr,
                                 solver.ptr, ws.ptr, nws, a['flags'], 0)
    assert err.value.status == -1                                             # PGX_ERR_INVALID
    torch.cuda.synchronize()
    assert table.is_still_garbage() and solver.is_still_garbage() and ws.is_still_garbage()
    # the host entry refuses the same arguments (its table is the loaded one: the shapes cannot be wrong there)
    if 'G' not in bad and 'S' not in bad:
        gpu_ctx.bernoulli_load(z['rows'], z['cols'], *X.shape)
        out = np.full((1 + sum(X.shape), 4), 7.0)
        rc = _native.lib().pgx_bernoulli_cd(gpu_ctx.handle, _native._ptr(host.start_point(z)), float(a['init_q']),
                                            float(a['lo']), float(a['hi']), min(a['T'], 2 ** 31), a['flags'],
                                            _native._ptr(out) if a['T'] == 3 else None, None)
        assert rc == -1 and np.all(out == 7.0)


def test_host_entry_refuses_a_start_point_outside_the_bounds_and_a_small_workspace(gpu_ctx):
    z = host.fixture('g64_s7')
    X = model.dense(z['rows'], z['cols'], z['shape'])
    G, S = X.shape
    gpu_ctx.bernoulli_load(z['rows'], z['cols'], G, S)
    for value in (0.5, 1.0, np.nan, np.inf):
        p0 = host.start_point(z)
        p0[3] = value
        with pytest.raises(_native.PgxError, match='init_p') as err:
            gpu_ctx.bernoulli_cd(p0, 0.9999, 0.8, 0.99999999, 2)
        assert err.value.status == -1
    nws = cd_ws_bytes(G, S)
    d_bits, d_p = chk.upload(bitmap(X)), chk.upload(host.start_point(z))
    table, ws = chk.guarded((1 + G + S) * 3 * 8, 0xFF), chk.guarded(nws, 0xFF)
    with pytest.raises(_native.PgxError, match='workspace too small'):
        gpu_ctx.bernoulli_cd_dev(d_bits.ptr, G, S, d_p.ptr, 0.9999, 0.8, 0.99999999, 2, table.ptr, None, ws.ptr, nws - 1, 0, 0)
    torch.cuda.synchronize()
    assert table.is_still_garbage() and ws.is_still_garbage()


@pytest.mark.parametrize('use_logs', [False, True])
def test_no_iterations_return_the_start_point_and_its_likelihood(use_logs, gpu_ctx):
    z = host.fixture('g70_s9_iter0' + ('_logs' if use_logs else ''))
    X = model.dense(z['rows'], z['cols'], z['shape'])
    G, S = X.shape
    gpu_ctx.bernoulli_load(z['rows'], z['cols'], G, S)
    p0 = host.start_point(z)
    table, solver = gpu_ctx.bernoulli_cd(p0, 0.9999, 0.8, 0.99999999, 0, use_logs=use_logs, solver_table=True)
    assert table.shape == (1 + G + S, 1)
    start = np.concatenate((p0, np.full(S, 0.9999)))
    if use_logs:
        np.testing.assert_allclose(solver[1:, 0], np.log(start), rtol=2.0 ** -52, atol=0)
        np.testing.assert_allclose(table[1:, 0], start, rtol=4 * 2.0 ** -52, atol=0)
    else:
        assert table[1:, 0].tobytes() == start.tobytes()
    assert_ll_at_own_variables(X, table, solver, use_logs)
    host.assert_table_matches_the_fixture(table, z, model.TOL)


# ---- 6. one sweep at the shapes that exercise the tiling, against the model -------------------------------------------
@pytest.mark.parametrize('name', ['g2000_s60', 'g4100_s5'])
@pytest.mark.parametrize('use_logs', [False, True])
def test_one_sweep_against_the_model(name, use_logs, gpu_ctx):
    """2000 x 60: 32 workgroups of genes in the row sweep; 4100 x 5: 65 bitmap words, a ragged last one (4 genes), in
    the column solve. One iteration from the fixture's start point: P and Q within TOL of the model (both satisfy
    Brent's stopping rule for the same computed f), the boundary branch in the same solves, LL at the device's own
    variables."""
    z = host.fixture(name + ('_logs' if use_logs else ''))
    X = model.dense(z['rows'], z['cols'], z['shape'])
    G, S = X.shape
    lo, hi = (float(v) for v in z['prob_bounds'])
    p0, icp = host.start_point(z), float(z['init_capture_prob'])
    gpu_ctx.bernoulli_load(z['rows'], z['cols'], G, S)
    table, solver = gpu_ctx.bernoulli_cd(p0, icp, lo, hi, 1, use_logs=use_logs, solver_table=True)
    want = model.run(X, p0, icp, lo, hi, 1, use_logs)
    worst = float(np.abs(table[1:] - want.table[1:]).max())
    print('largest |P, Q - model| %.3g (tolerance %.3g)' % (worst, model.TOL))
    assert worst <= model.TOL
    blo, bhi = (np.log(lo), np.log(hi)) if use_logs else (lo, hi)
    at_bound = (np.abs(solver[1:, 1] - blo) <= np.spacing(abs(blo))) | (np.abs(solver[1:, 1] - bhi) <= np.spacing(abs(bhi)))
    np.testing.assert_array_equal(at_bound[want.boundary[0]], True)
    assert_ll_at_own_variables(X, table, solver, use_logs)
    stats = gpu_ctx.bernoulli_cd_stats()
    assert stats['not_converged'] == 0 and stats['solves'] == G + S
    print('evaluations per solve: mean %.2f max %d (model: mean %.2f max %d)'
          % (stats['evaluations'] / float(G + S), stats['max_evaluations'], want.evals.mean(), want.evals.max()))
