"""The Bernoulli likelihood kernels at the edges of their values: tables without (or almost without) absent cells, points
on the bounds, and both sides of the switch between the fast mode and the per-cell expressions. The yardstick is
tests/bernoulli_model.py's evaluate(), and for the two fixtures of tests/golden/bernoulli_edges the reference itself
(tests/golden/make_golden_bernoulli_edges.py).

LL tolerance (bernoulli_model.ll_bound_reference): 1e-12 x ll_scale + 2 u x (present cells), u = 2^-53. On a table
without absent cells near the upper bound |log(p q)| is about 1e-8 per cell while log(fl(p q)) carries an absolute
error of up to u per cell, so rtol 1e-12 on LL cannot hold between the reference's per-cell sum and the fast mode's
rowsum log p + colsum log q -- the fast mode being the accurate one (test_bernoulli_host.py, against 50 digits).
Gradient entries: 1e-12 x the sum of the absolute values of their terms. Specials exactly where evaluate() has them."""
import contextlib
import glob
import io
import os

import numpy as np
import pytest

import bernoulli_model as bm
from pangenomix_amd import pangenome_analysis as pa
from test_gpu_bernoulli import assert_same_specials, dense_frame
from test_gpu_bernoulli_geometry import LoadedTable

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = sorted(glob.glob(os.path.join(HERE, 'golden', 'bernoulli_edges', '*.npz')))
FIXTURE_IDS = [os.path.basename(p)[:-4] for p in FIXTURES]
TINY = 2.0 ** -511                                           # TINY * TINY: the smallest normal number


def check_both_modes(table, pq, label):
    """Both modes through every entry against evaluate(); where evaluate() is finite and every product lies inside
    (0, 1), fast mode against PGX_BERNOULLI_EXACT within the same bounds. Returns (evaluation, fast LL - exact LL)."""
    ev = bm.evaluate(table.X, pq)
    fast, exact = (table.eval_all_entries(pq, mode) for mode in (False, True))
    for out, mode in ((fast, 'fast'), (exact, 'exact')):
        bm.assert_evaluation(out, ev, (label, mode))
    with np.errstate(all='ignore'):
        r = np.outer(pq[:table.G], pq[table.G:])
        inside = bool(np.all((r > 0) & (r < 1)))
    if np.isfinite(ev.ll) and np.all(np.isfinite(ev.grad)) and inside:
        assert abs(fast[0] - exact[0]) <= bm.ll_bound_reference(ev), (label, fast[0] - exact[0])
        assert np.all(np.abs(fast[1:] - exact[1:]) <= 1e-12 * ev.scale), label
    return ev, fast[0] - exact[0]


@pytest.mark.parametrize('G,S', bm.EDGE_SHAPES)
def test_edge_tables_at_edge_points(G, S, gpu_ctx):
    """All ones, all zeros, one zero in an all-ones table, one all-ones column; at the start point, everything on the
    upper bound, everything on the lower bound, and P, Q in [0.9999999, 0.99999999]."""
    for name, X in bm.edge_tables(G, S).items():
        table = LoadedTable(gpu_ctx, X)
        for point, pq in bm.edge_points(X).items():
            ev, diff = check_both_modes(table, pq, (name, point))
            assert np.isfinite(ev.ll)
            print('%d x %d %s at %s: LL %.17g, fast - exact %.3g (relative %.3g; bound %.3g)'
                  % (G, S, name, point, ev.ll, diff, abs(diff / ev.ll) if ev.ll else 0.0, bm.ll_bound_reference(ev)))


def boundary_table(present):
    """65 x 7, half of the cells absent; the cell (I, J) whose product the cases below put on a boundary is present or
    absent."""
    X = np.random.default_rng(65).random((65, 7)) < 0.5
    X[BOUNDARY_I, BOUNDARY_J] = present
    return X


BOUNDARY_I, BOUNDARY_J = 64, 3                              # the last gene: the one valid bit of the last word


def boundary_point(p_range, q_range, p=None, q=None):
    rng = np.random.default_rng(9)
    pq = np.concatenate((rng.uniform(p_range[0], p_range[1], 65), rng.uniform(q_range[0], q_range[1], 7)))
    if p is not None:
        pq[BOUNDARY_I] = p
    if q is not None:
        pq[65 + BOUNDARY_J] = q
    return pq


INTERIOR = ((0.8, 0.99), (0.8, 0.99))
HALVES = ((0.3, 0.5), (1.5, 2.0))                            # P <= 0.5, Q <= 2: the largest product is 0.5 x 2.0
BOUNDARY_POINTS = {
    'max_product_1x1': boundary_point(*INTERIOR, p=1.0, q=1.0),
    'max_product_below_1x1': boundary_point(*INTERIOR, p=np.nextafter(1.0, 0.0), q=1.0),
    'max_product_half_x_2': boundary_point(*HALVES, p=0.5, q=2.0),
    'max_product_below_half_x_2': boundary_point(*HALVES, p=0.5, q=np.nextafter(2.0, 0.0)),
    'min_product_rounds_to_0': boundary_point(*INTERIOR, p=1e-162, q=1e-162),
    'min_product_subnormal': boundary_point(*INTERIOR, p=1e-161, q=1e-161),
    'min_product_smallest_normal': boundary_point(*INTERIOR, p=TINY, q=TINY),
    'min_product_largest_subnormal_step': boundary_point(*INTERIOR, p=TINY, q=0.75 * TINY),
    'nan_in_P': boundary_point(*INTERIOR, p=np.nan),
    'inf_in_P': boundary_point(*INTERIOR, p=np.inf),
    'negative_in_P': boundary_point(*INTERIOR, p=-0.5),
    'nan_in_Q': boundary_point(*INTERIOR, q=np.nan),
    'inf_in_Q': boundary_point(*INTERIOR, q=np.inf),
    'negative_in_Q': boundary_point(*INTERIOR, q=-0.5),
}
# LL as evaluate() must give it when the cell (I, J) is present / absent (the per-cell expressions of pgx.h)
BOUNDARY_LL = {
    'max_product_1x1': ('nan', '-inf'),                      # log 1 + 0 * log 0; 0 * log 1 + log 0
    'max_product_below_1x1': ('finite', 'finite'),
    'max_product_half_x_2': ('nan', '-inf'),
    'max_product_below_half_x_2': ('finite', 'finite'),
    'min_product_rounds_to_0': ('-inf', 'nan'),              # log 0 + 0 * log 1; 0 * log 0 + log 1
    'min_product_subnormal': ('finite', 'finite'),
    'min_product_smallest_normal': ('finite', 'finite'),
    'min_product_largest_subnormal_step': ('finite', 'finite'),
}


def kind_of(v):
    return 'finite' if np.isfinite(v) else str(float(v))


@pytest.mark.parametrize('present', [True, False], ids=['cell_present', 'cell_absent'])
@pytest.mark.parametrize('case', sorted(BOUNDARY_POINTS))
def test_both_sides_of_the_mode_switch(case, present, gpu_ctx):
    """pmax qmax == 1 against the next double below; pmin qmin rounding to 0 against a subnormal product, and the
    smallest normal product against a subnormal one (the fast mode is left below the smallest normal number: a
    subnormal fl(p q) has lost bits, 0.012 in the log of fl(1e-161 x 1e-161)); a nan, a +inf and a negative entry in
    P and in Q."""
    table = LoadedTable(gpu_ctx, boundary_table(present))
    ev, diff = check_both_modes(table, BOUNDARY_POINTS[case], (case, present))
    if case in BOUNDARY_LL:
        assert kind_of(ev.ll) == BOUNDARY_LL[case][0 if present else 1]
    else:
        assert np.isnan(ev.ll)
    print('%s, cell %s: LL %r, fast - exact %r' % (case, 'present' if present else 'absent', float(ev.ll), float(diff)))


def recorded_bound(z, k):
    return 1e-12 * z['point_ll_scale'][k] + 2 * bm.U * z['rows'].size


@pytest.mark.parametrize('path', FIXTURES, ids=FIXTURE_IDS)
def test_evaluations_match_the_reference_on_tables_without_absent_cells(path, gpu_ctx):
    z = np.load(path)
    G, S = (int(v) for v in z['shape'])
    X = np.zeros((G, S), dtype=bool)
    X[z['rows'], z['cols']] = True
    table = LoadedTable(gpu_ctx, X)
    for k, pt in enumerate(z['points']):
        for exact in (False, True):
            out = table.eval_all_entries(pt, exact)
            err = abs(out[0] - z['point_ll'][k])
            print('%s point %d %s: LL %.17g, reference %.17g, difference %.3g (relative %.3g; bound %.3g)'
                  % (os.path.basename(path), k, 'exact' if exact else 'fast', out[0], z['point_ll'][k], err,
                     err / abs(z['point_ll'][k]), recorded_bound(z, k)))
            assert err <= recorded_bound(z, k)
            assert np.all(np.abs(out[1:] - z['point_grad'][k]) <= 1e-12 * z['point_scale'][k])


@pytest.mark.parametrize('path', FIXTURES, ids=FIXTURE_IDS)
def test_whole_call_matches_the_reference_on_tables_without_absent_cells(path, gpu_ctx):
    """The reference's nit, nfev and status, x within 1e-7, and the initial and final LL within the evaluation's bound at
    those two points (points[0] is the start point, points[1] the reference's optimum)."""
    z = np.load(path)
    with contextlib.redirect_stdout(io.StringIO()):
        df_opt, res = pa.compute_bernoulli_grid_core_genome(dense_frame(z), ctx=gpu_ctx)
    assert list(df_opt.index) == list(z['labels'])
    init, opt = df_opt['initial'].values, df_opt['optimum'].values
    assert_same_specials(init, z['initial'])
    np.testing.assert_allclose(init[1:], z['initial'][1:], rtol=1e-12, atol=0)
    assert (res.nit, res.nfev, res.status) == (int(z['nit']), int(z['nfev']), int(z['status']))
    np.testing.assert_allclose(res.x, z['x'], rtol=0, atol=1e-7)
    np.testing.assert_allclose(opt[1:], z['optimum'][1:], rtol=0, atol=1e-7)
    print('%s: initial LL %.17g (reference %.17g), optimum %.17g (reference %.17g)'
          % (os.path.basename(path), init[0], z['initial'][0], opt[0], z['optimum'][0]))
    assert abs(init[0] - z['initial'][0]) <= recorded_bound(z, 0)
    assert abs(opt[0] - z['optimum'][0]) <= recorded_bound(z, 1)
