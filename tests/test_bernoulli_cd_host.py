"""compute_bernoulli_grid_core_genome_cd without a GPU: the numpy model (tests/bernoulli_cd_model.py: the device's order of
summation and Brent driver) against every fixture of the reference (tests/golden/bernoulli_cd, written by
tests/golden/make_golden_bernoulli_cd.py), the refusals that happen before any library call, and labels, columns and prints
of the Python entry through a stand-in context that answers with the model.

Tolerances: P and Q within bernoulli_cd_model.TOL = 2 (xtol + rtol) = 4.1e-12 of the reference on the
device; that tolerance stands only while the MODEL differs from the reference by less than a tenth of it, which is what
is asserted here for every fixture (measured: 1.2e-16). LL under DESIGN.md 6a's rule, 1e-12 x (sum of absolute terms) +
2^-52 x (present cells), plus what the tolerated movement of P and Q does to it: sum_k |dLL/dx_k| x TOL."""
import contextlib
import glob
import io
import os

import numpy as np
import pandas as pd
import pytest
import scipy.sparse

import bernoulli_cd_model as model
from pangenomix_amd import _native, sparse_utils
from pangenomix_amd import pangenome_analysis as pa

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = sorted(glob.glob(os.path.join(HERE, 'golden', 'bernoulli_cd', '*.npz')))
IDS = [os.path.basename(p)[:-4] for p in FIXTURES]


def fixture(name):
    return np.load(os.path.join(HERE, 'golden', 'bernoulli_cd', name + '.npz'))


def dense_frame(z):
    X = model.dense(z['rows'], z['cols'], z['shape']).astype(str(z['dtype']))
    return pd.DataFrame(X, index=list(z['index']), columns=list(z['columns']))


def lsdf(z):
    G, S = (int(v) for v in z['shape'])
    m = scipy.sparse.coo_matrix((np.ones(z['rows'].size, dtype=np.int64), (z['rows'], z['cols'])), shape=(G, S))
    return sparse_utils.LightSparseDataFrame(list(z['index']), list(z['columns']), m)


def call_args(z):
    freqs = z['init_gene_freqs']
    return dict(n_iterations=int(z['n_iterations']), prob_bounds=tuple(float(v) for v in z['prob_bounds']),
                init_capture_prob=float(z['init_capture_prob']), init_gene_freqs=None if freqs.size == 0 else freqs,
                use_logs=bool(z['use_logs']))


def start_point(z):
    G, S = (int(v) for v in z['shape'])
    freqs = z['init_gene_freqs']
    P = np.bincount(z['rows'], minlength=G) / float(S) if freqs.size == 0 else freqs
    return np.clip(P, z['prob_bounds'][0], z['prob_bounds'][1])


def ll_tolerance(X, column, use_logs):
    """Against the fixture's LL: the tolerated movement of every P and Q through the gradient at the fixture's point
    (taken in p and q: the table holds them in both flavours), plus the accuracy rule of the sum itself."""
    grad = model.ll_gradient(X, column[1:], False)
    _, scale, present = model.likelihood(X, column[1:], False)
    return float(np.abs(grad).sum()) * model.TOL + model.ll_bound(scale, present)


def assert_table_matches_the_fixture(table, z, tol):
    """P and Q of every iteration within tol; LL within ll_tolerance"""
    X = model.dense(z['rows'], z['cols'], z['shape'])
    want = z['table']
    assert table.shape == want.shape
    worst = float(np.abs(table[1:] - want[1:]).max())
    print('largest |P, Q - reference| %.3g (tolerance %.3g)' % (worst, tol))
    assert worst <= tol
    for k in range(want.shape[1]):
        bound = ll_tolerance(X, want[:, k], bool(z['use_logs']))
        print('column %d: |LL - reference| %.3g (bound %.3g)' % (k, abs(table[0, k] - want[0, k]), bound))
        assert abs(table[0, k] - want[0, k]) <= bound
    return worst


def assert_printed_matches_the_fixture(text, table, z):
    """The same lines; the numbers are the table's row 0 (their bounds are checked on the table)"""
    lines, want = text.splitlines(), list(z['printed'])
    assert [ln.split(':')[0] for ln in lines] == [ln.split(':')[0] for ln in want]
    lls = [float(ln.split(':')[1]) for ln in lines if 'oglikelihood' in ln]
    assert lls == [float(v) for v in table[0]]
    assert [ln for ln in lines if ln.startswith('Iteration')] == [ln for ln in want if ln.startswith('Iteration')]
    assert lines[0].startswith('Initial Loglikelihood:' if bool(z['use_logs']) else 'Loglikelihood:')


@pytest.mark.parametrize('path', FIXTURES, ids=IDS)
def test_model_reproduces_the_references_fixtures(path):
    """The tenth of the tolerance that lets the device be held to TOL, the boundary branch in the same solves, no solve
    that fails, LL within its bound."""
    z = np.load(path)
    lo, hi = (float(v) for v in z['prob_bounds'])
    X = model.dense(z['rows'], z['cols'], z['shape'])
    run = model.run(X, start_point(z), float(z['init_capture_prob']), lo, hi, int(z['n_iterations']), bool(z['use_logs']))
    assert_table_matches_the_fixture(run.table, z, model.TOL / 10)
    assert not run.failed.any()
    np.testing.assert_array_equal(run.boundary, z['boundary'])
    assert int(run.evals.max(initial=2)) <= 2 + model.MAXITER
    on_bound = run.boundary
    solved = run.solver[1:, 1:].T
    blo, bhi = (np.log(lo), np.log(hi)) if bool(z['use_logs']) else (lo, hi)
    assert np.all((solved[on_bound] == blo) | (solved[on_bound] == bhi))
    assert np.all((solved >= blo) & (solved <= bhi))


def test_fixtures_cover_the_cases():
    names = set(IDS)
    for shape in ('g63_s1', 'g64_s7', 'g65_s63', 'g128_s64', 'g129_s65', 'g2000_s60', 'g4100_s5', 'g5_s300', 'g1_s1',
                  'g70_s9_iter0', 'g70_s9_freqs', 'g70_s9_bounds', 'g70_s9_icp1', 'g70_s9_float64'):
        assert shape in names and shape + '_logs' in names
    z = fixture('g70_s9_freqs')
    lo, hi = z['prob_bounds']
    assert (z['init_gene_freqs'] < lo).any() and (z['init_gene_freqs'] > hi).any()
    assert str(fixture('g70_s9_float64')['dtype']) == 'float64' and str(z['dtype']) == 'int64'
    # both branches are taken, and the recorder's conditions hold on what is committed
    for path in FIXTURES:
        z = np.load(path)
        if int(z['n_iterations']) == 0:
            continue
        live = ~z['trivial']
        if live.any():
            margin = np.minimum(np.abs(z['f_lo']) / z['scale_lo'], np.abs(z['f_hi']) / z['scale_hi'])[live]
            assert margin.min() >= 1e-9
    assert any(np.load(p)['boundary'].any() and not np.load(p)['boundary'].all() for p in FIXTURES)


# ---- the Python entry: refusals before any library call ---------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError('the library was called before the input was checked')
    monkeypatch.setattr(_native, 'lib', refuse)
    monkeypatch.setattr(_native, 'default_context', refuse)


def small_frame():
    return pd.DataFrame(np.array([[1, 1, 0], [1, 0, 1], [1, 1, 1]]), index=list('abc'), columns=list('xyz'))


@pytest.mark.parametrize('kwargs', [
    dict(prob_bounds=(0.0, 0.9)), dict(prob_bounds=(-0.1, 0.9)), dict(prob_bounds=(0.9, 0.9)), dict(prob_bounds=(0.9, 0.8)),
    dict(prob_bounds=(0.8, 1.0)), dict(prob_bounds=(0.8, 1.5)), dict(prob_bounds=(0.8, np.nan)),
    dict(prob_bounds=(np.nan, 0.9)), dict(prob_bounds=(0.8, np.inf)), dict(prob_bounds=(0.8,)),
    dict(init_capture_prob=0.0), dict(init_capture_prob=-0.5), dict(init_capture_prob=np.nan),
    dict(init_capture_prob=np.inf), dict(init_capture_prob=2.0),
    dict(prob_bounds=(0.5, 0.9), init_capture_prob=1.2),
    dict(n_iterations=-1), dict(n_iterations=2.5), dict(n_iterations=2 ** 20 + 1),
    dict(init_gene_freqs=[0.9, 0.9]), dict(init_gene_freqs=[0.9, np.nan, 0.9]), dict(init_gene_freqs=[0.9, np.inf, 0.9]),
    dict(init_gene_freqs=['a', 'b', 'c']),
])
def test_arguments_outside_the_contract_are_refused(no_library, kwargs):
    with pytest.raises(ValueError, match='compute_bernoulli_grid_core_genome_cd'):
        pa.compute_bernoulli_grid_core_genome_cd(small_frame(), **kwargs)


@pytest.mark.parametrize('shape', [(0, 3), (3, 0), (0, 0)])
def test_an_empty_table_is_refused(no_library, shape):
    frame = pd.DataFrame(np.zeros(shape, dtype=np.int64), index=list('abc')[:shape[0]], columns=list('xyz')[:shape[1]])
    with pytest.raises(ValueError, match='compute_bernoulli_grid_core_genome_cd'):
        pa.compute_bernoulli_grid_core_genome_cd(frame)


def test_tables_that_are_not_binary_are_refused_in_this_functions_name(no_library):
    X = np.ones((5, 3))
    X[2, 1] = 2
    with pytest.raises(ValueError, match='compute_bernoulli_grid_core_genome_cd needs a binary'):
        pa.compute_bernoulli_grid_core_genome_cd(pd.DataFrame(X, index=list('abcde'), columns=list('xyz')))
    m = scipy.sparse.coo_matrix((np.ones(4, dtype=np.int64), ([0, 1, 2, 1], [0, 1, 1, 1])), shape=(3, 2))
    with pytest.raises(ValueError, match='compute_bernoulli_grid_core_genome_cd needs a table without duplicate'):
        pa.compute_bernoulli_grid_core_genome_cd(sparse_utils.LightSparseDataFrame(list('abc'), list('xy'), m))
    with pytest.raises(TypeError, match='compute_bernoulli_grid_core_genome_cd takes'):
        pa.compute_bernoulli_grid_core_genome_cd(np.ones((3, 2)))
    # the other entry keeps its own name
    with pytest.raises(ValueError, match='compute_bernoulli_grid_core_genome needs a binary'):
        pa.compute_bernoulli_grid_core_genome(pd.DataFrame(X, index=list('abcde'), columns=list('xyz')))


# ---- the Python entry through a stand-in context -----------------------------------------------------------------------
class ModelContext(object):
    """Answers bernoulli_load / bernoulli_cd with the numpy model; records what it was asked."""

    def __init__(self):
        self.calls = []

    def bernoulli_load(self, rows, cols, n_genes, n_genomes):
        self.X = model.dense(rows, cols, (n_genes, n_genomes))
        self.calls.append('load')
        return 0

    def bernoulli_cd(self, init_p, init_q, lo, hi, n_iterations, use_logs=False, solver_table=False):
        self.calls.append('cd')
        self.args = (np.array(init_p), init_q, lo, hi, n_iterations, use_logs)
        run = model.run(self.X, init_p, init_q, lo, hi, n_iterations, use_logs)
        return (run.table, run.solver) if solver_table else run.table


@pytest.mark.parametrize('name', ['g64_s7', 'g64_s7_logs', 'g70_s9_iter0', 'g70_s9_iter0_logs', 'g70_s9_freqs',
                                  'g70_s9_freqs_logs', 'g70_s9_bounds', 'g70_s9_icp1_logs', 'g70_s9_float64', 'g1_s1'])
def test_entry_returns_the_references_frame_and_prints(name):
    z = fixture(name)
    ctx = ModelContext()
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        df = pa.compute_bernoulli_grid_core_genome_cd(dense_frame(z), ctx=ctx, **call_args(z))
    assert ctx.calls == ['load', 'cd']                                    # one library call for the whole loop
    assert list(df.index) == list(z['labels'])
    assert list(df.columns) == list(range(int(z['n_iterations']) + 1)) and df.columns.dtype == np.arange(1).dtype
    assert df.values.dtype == np.float64
    assert_table_matches_the_fixture(df.values, z, model.TOL / 10)
    assert_printed_matches_the_fixture(buf.getvalue(), df.values, z)
    init_p, init_q, lo, hi, n_it, logs = ctx.args
    assert (lo, hi) == tuple(z['prob_bounds']) and init_q == float(z['init_capture_prob'])     # Q is not clipped
    assert np.all((init_p >= lo) & (init_p <= hi)) and np.array_equal(init_p, start_point(z))


def test_entry_takes_every_input_form():
    z = fixture('g64_s7')
    frames = [dense_frame(z), lsdf(z), lsdf(z).to_sparse_arrays()]
    tables = []
    for frame in frames:
        with contextlib.redirect_stdout(io.StringIO()):
            tables.append(pa.compute_bernoulli_grid_core_genome_cd(frame, ctx=ModelContext(), **call_args(z)))
    for t in tables[1:]:
        assert t.equals(tables[0])


def test_workspace_size_is_declared_and_grows_with_the_table():
    f = _native.lib().pgx_bernoulli_cd_workspace_bytes
    assert 0 < f(1, 1) <= f(64, 7) <= f(4100, 5) <= f(40000, 400)
    assert f(40000, 400) >= _native.lib().pgx_bernoulli_workspace_bytes(40000, 400) + 5 * 8 * 40400
