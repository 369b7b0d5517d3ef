#!/usr/bin/env python
"""Golden fixtures for compute_bernoulli_grid_core_genome (reference pangenome_analysis.py:101-166), produced by RUNNING
THE REFERENCE in the build container (needs /root/reference; it never travels to the GPU box):

    python tests/golden/make_golden_core.py

For every case, tests/golden/core/<case>.npz holds
  rows, cols, shape            the binary table as COO coordinates (int32) and its shape
  index, columns               its labels
  prob_bounds, init_capture_prob, init_gene_freqs (empty = None)
  initial, optimum             the two columns of the reference's df_opt_full; labels = its index
  x, fun, nit, nfev, status    of the reference's OptimizeResult
  printed                      the lines the call printed (its own prints; what scipy prints from Python)
  points                       [k, n_genes + n_genomes] points (P; Q) at which the reference's own likelihood and
  point_ll, point_grad         gradient functions were evaluated (the start point, the optimum, an interior point and
                               a point with entries on both bounds)
  point_scale                  per gradient entry: the sum of the absolute values of its terms (|rowsum_i / p_i| +
                               sum_j |(1 - X_ij) q_j / (1 - p_i q_j)|, likewise for q), which scales its tolerance;
                               and per point the sum of the absolute LL terms (point_ll_scale)

`pangenome_analysis` imports statsmodels.stats at module level; it is not installed and not used by this function, so
an EMPTY placeholder module is registered under that name (as make_golden_next.py does).
"""
import contextlib
import io
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, '/root/reference')
sys.path.insert(0, '/root/reference/pangenomix')
for _name in ('statsmodels', 'statsmodels.stats'):
    sys.modules.setdefault(_name, types.ModuleType(_name))
sys.modules['statsmodels'].stats = sys.modules['statsmodels.stats']

import pandas as pd                                       # noqa: E402
import pangenomix.pangenome_analysis as ref_pa            # noqa: E402

ref_ll = getattr(ref_pa, '__bernoulli_grid_loglikelihood__')
ref_grad = getattr(ref_pa, '__bernoulli_grid_loglikelihood_gradient__')


def table(rng, G, S, ones_row=None, zeros_row=None):
    p = rng.uniform(0.85, 1.0, G)
    q = rng.uniform(0.95, 1.0, S)
    X = (rng.random((G, S)) < np.outer(p, q)).astype(np.int64)
    if ones_row is not None:
        X[ones_row] = 1
    if zeros_row is not None:
        X[zeros_row] = 0
    return X


def scales(X, P, Q):
    """Sum of absolute terms of every gradient entry and of LL (this generator's own restatement)."""
    with np.errstate(all='ignore'):
        r = np.outer(P, Q)
        t = 1.0 - r
        absent = (X == 0)
        gp = np.abs(X.sum(1) / P) + np.where(absent, np.abs(Q[None, :] / t), 0.0).sum(1)
        gq = np.abs(X.sum(0) / Q) + np.where(absent, np.abs(P[:, None] / t), 0.0).sum(0)
        ll = np.where(absent, np.abs(np.log(t)), np.abs(np.log(r))).sum()
    return np.concatenate((gp, gq)), ll


CASES = [
    # name, G, S, seed, extra
    ('g65_s7', 65, 7, 1, {}),
    ('g63_s1', 63, 1, 2, {}),
    ('g128_s12_rows', 128, 12, 3, {'ones_row': 5, 'zeros_row': 77}),
    ('g100_s9_freqs', 100, 9, 4, {'freqs': True, 'init_capture_prob': 0.99}),
    ('g2000_s60', 2000, 60, 5, {}),
    ('g50_s12_nan', 50, 12, 6, {'prob_bounds': (0.8, 1.0), 'init_capture_prob': 1.0}),
]


def main():
    out = os.path.join(HERE, 'core')
    os.makedirs(out, exist_ok=True)
    for name, G, S, seed, extra in CASES:
        rng = np.random.default_rng(seed)
        X = table(rng, G, S, extra.get('ones_row'), extra.get('zeros_row'))
        index = ['gene%d' % i for i in range(G)]
        columns = ['genome%d' % j for j in range(S)]
        df = pd.DataFrame(X, index=index, columns=columns)
        bounds = extra.get('prob_bounds', (0.8, 0.99999999))
        icp = extra.get('init_capture_prob', 0.9999)
        freqs = rng.uniform(0.7, 1.0, G) if extra.get('freqs') else None
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf), warnings.catch_warnings():
            warnings.simplefilter('ignore')
            df_opt, res = ref_pa.compute_bernoulli_grid_core_genome(df, prob_bounds=bounds, init_capture_prob=icp,
                                                                    init_gene_freqs=freqs)
        printed = buf.getvalue().splitlines()
        start = df_opt['initial'].values[1:]
        lo, hi = bounds
        interior = rng.uniform(lo, lo + 0.999 * (hi - lo), G + S)
        edges = rng.uniform(lo, hi, G + S)
        edges[::3] = lo
        edges[1::3] = hi
        points = np.stack([start, np.asarray(res.x), interior, edges])
        lls, grads, gscale, llscale = [], [], [], []
        for pt in points:
            with warnings.catch_warnings(), np.errstate(all='ignore'):
                warnings.simplefilter('ignore')
                lls.append(ref_ll(X, pt[:G], pt[G:]))
                grads.append(ref_grad(X, pt[:G], pt[G:]))
            gs, ls = scales(X, pt[:G], pt[G:])
            gscale.append(gs)
            llscale.append(ls)
        r, c = np.nonzero(X)
        np.savez_compressed(os.path.join(out, name + '.npz'), rows=r.astype(np.int32), cols=c.astype(np.int32),
                            shape=np.array([G, S], dtype=np.int64), index=np.array(index), columns=np.array(columns),
                            prob_bounds=np.array(bounds, dtype=np.float64), init_capture_prob=np.float64(icp),
                            init_gene_freqs=np.zeros(0) if freqs is None else freqs,
                            labels=np.array(df_opt.index.tolist()), initial=df_opt['initial'].values,
                            optimum=df_opt['optimum'].values, x=np.asarray(res.x), fun=np.float64(res.fun),
                            nit=np.int64(res.nit), nfev=np.int64(res.nfev), status=np.int64(res.status),
                            printed=np.array(printed), points=points, point_ll=np.array(lls),
                            point_grad=np.array(grads), point_scale=np.array(gscale),
                            point_ll_scale=np.array(llscale))
        print('%s: %dx%d LL %r -> %r nit %d nfev %d status %d' % (name, G, S, df_opt['initial'].values[0], -res.fun,
                                                                  res.nit, res.nfev, res.status))

    # the reference's LightSparseDataFrame.to_sparse_arrays() frame of a small table: dtypes, stored entries, fill
    import pangenomix.sparse_utils as ref_su
    import scipy.sparse
    rng = np.random.default_rng(7)
    X = table(rng, 70, 5, ones_row=3, zeros_row=9)
    X[11, 2] = 0
    r, c = np.nonzero(X)
    m = scipy.sparse.coo_matrix((np.ones(r.size, dtype=np.int64), (r, c)), shape=X.shape)
    lsdf = ref_su.LightSparseDataFrame(['g%d' % i for i in range(70)], ['s%d' % j for j in range(5)], m)
    frame = lsdf.to_sparse_arrays()
    arrays = {}
    for j, col in enumerate(frame.columns):
        a = frame[col].array
        arrays['sp_values_%d' % j] = np.asarray(a.sp_values)
        arrays['sp_indices_%d' % j] = np.asarray(a.sp_index.indices)
    np.savez_compressed(os.path.join(out, 'to_sparse_arrays.npz'), rows=r.astype(np.int32), cols=c.astype(np.int32),
                        shape=np.array(X.shape, dtype=np.int64), index=np.array(list(frame.index)),
                        columns=np.array(list(frame.columns)), dtypes=np.array([str(t) for t in frame.dtypes]),
                        fill_is_nan=np.array([bool(np.isnan(frame[c].array.fill_value)) for c in frame.columns]),
                        kinds=np.array([frame[c].array.kind for c in frame.columns]), **arrays)
    print('to_sparse_arrays: %d columns %s' % (frame.shape[1], sorted(set(str(t) for t in frame.dtypes))))


if __name__ == '__main__':
    main()
