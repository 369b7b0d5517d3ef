#!/usr/bin/env python
"""Golden fixtures for compute_bernoulli_grid_core_genome_cd (reference pangenome_analysis.py:169-242, helpers :251-292),
produced by RUNNING THE REFERENCE in the build container (needs /root/reference; it never travels to the GPU box):

    python tests/golden/make_golden_bernoulli_cd.py

For every case, tests/golden/bernoulli_cd/<case>.npz holds
  rows, cols, shape            the binary table as COO coordinates (int32) and its shape
  index, columns, dtype        its labels and the dtype of the dense frame the reference was given
  n_iterations, prob_bounds, init_capture_prob, init_gene_freqs (empty = None), use_logs
  table, labels                the array the reference returned and its index
  printed                      the lines the call printed
  f_lo, f_hi                   per solve, [n_iterations, n_genes + n_genomes] (genes first), float32: the value of the
  scale_lo, scale_hi           solve's function at the two bounds and the sum of its absolute terms there
                               (|rowsum / p| + sum |terms|), in the solver's variable
  boundary                     whether the solve took the boundary branch (f(lo) f(hi) >= 0)
  trivial                      whether the solve's row / column is present everywhere or nowhere
The per-solve records come from wrapping the reference's two helper functions: the wrapper evaluates the function at the
bounds with the expression of DESIGN.md 6g and then calls the helper itself.

Two conditions are asserted for every case (a case that breaks one gets another seed; the conditions stay):
  (a) in every solve that is not trivial, |f(bound)| >= 1e-9 x scale at both bounds: summation noise is at most
      n 2^-53 x scale = 4.6e-13 x scale for n <= 4,100, so no order of summation can flip the test f(lo) f(hi) >= 0
  (b) in every solve that takes the boundary branch, | |last - lo| - |last - hi| | >= 1e-9
Their smallest margins are printed per case, and so is the largest difference between tests/bernoulli_cd_model.py and the
reference over P and Q of every iteration (DESIGN.md 6g quotes both).

`pangenome_analysis` imports statsmodels.stats at module level; it is not installed and not used by this function, so
an EMPTY placeholder module is registered under that name (as make_golden_core.py does).
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
sys.path.insert(0, os.path.dirname(HERE))
for _name in ('statsmodels', 'statsmodels.stats'):
    sys.modules.setdefault(_name, types.ModuleType(_name))
sys.modules['statsmodels'].stats = sys.modules['statsmodels.stats']

import pandas as pd                                       # noqa: E402
import pangenomix.pangenome_analysis as ref_pa            # noqa: E402
import bernoulli_cd_model as model                        # noqa: E402

PLAIN, LOGS = '__bernoulli_grid_coordinate_descent__', '__bernoulli_grid_coordinate_descent_from_logs__'


def table(rng, G, S, ones_row=None, zeros_row=None, ones_col=None):
    """make_golden_core.py's recipe"""
    p = rng.uniform(0.85, 1.0, G)
    q = rng.uniform(0.95, 1.0, S)
    X = (rng.random((G, S)) < np.outer(p, q)).astype(np.int64)
    if ones_row is not None:
        X[ones_row] = 1
    if zeros_row is not None:
        X[zeros_row] = 0
    if ones_col is not None:
        X[:, ones_col] = 1
    return X


class Recorder(object):
    """Wraps one of the reference's helpers: records every solve, then calls the helper."""

    def __init__(self, helper, use_logs):
        self.helper, self.use_logs, self.solves = helper, use_logs, []

    def __call__(self, Xk, other, last, bounds):
        lo, hi = float(bounds[0]), float(bounds[1])
        absent = (Xk == 0)
        n = float(Xk.sum())
        rec = []
        for x in (lo, hi):
            if self.use_logs:
                terms = np.where(absent, np.exp(other) / (-np.expm1(x + other)), 0.0)
                head = n * np.exp(-x)
            else:
                terms = np.where(absent, other / (1.0 - x * other), 0.0)
                head = n / x
            rec += [head - terms.sum(), abs(head) + np.abs(terms).sum()]
        f_lo, s_lo, f_hi, s_hi = rec
        boundary = f_lo * f_hi >= 0
        trivial = bool(absent.all() or not absent.any())
        if not trivial:                                                                   # condition (a)
            assert abs(f_lo) >= 1e-9 * s_lo and abs(f_hi) >= 1e-9 * s_hi, ('condition (a)', f_lo, s_lo, f_hi, s_hi)
        side = abs(abs(last - lo) - abs(last - hi))
        if boundary:                                                                      # condition (b)
            assert side >= 1e-9, ('condition (b)', last, lo, hi)
        out = self.helper(Xk, other, last, bounds)
        if boundary:
            assert out == lo or out == hi
        self.solves.append((f_lo, f_hi, s_lo, s_hi, boundary, trivial, side))
        return out


SHAPES = [
    # name, G, S, iterations, seed, special rows / columns
    ('g63_s1', 63, 1, 3, 11, {'ones_row': 1, 'zeros_row': 2}),
    ('g64_s7', 64, 7, 3, 12, {'ones_row': 1, 'zeros_row': 2}),
    ('g65_s63', 65, 63, 3, 13, {'ones_row': 1, 'ones_col': 1}),
    ('g128_s64', 128, 64, 3, 14, {'ones_row': 1, 'zeros_row': 2}),
    ('g129_s65', 129, 65, 3, 15, {'ones_row': 1, 'ones_col': 1}),
    ('g2000_s60', 2000, 60, 3, 16, {'ones_row': 1, 'zeros_row': 2}),
    ('g4100_s5', 4100, 5, 2, 17, {'ones_row': 1, 'zeros_row': 2}),
    ('g5_s300', 5, 300, 3, 18, {'ones_row': 1, 'ones_col': 1}),
    ('g1_s1', 1, 1, 2, 19, {}),
]
CASES = [(name + ('_logs' if logs else ''), G, S, seed, dict(special), dict(n_iterations=it, use_logs=logs))
         for name, G, S, it, seed, special in SHAPES for logs in (False, True)]
for _logs in (False, True):
    _t = '_logs' if _logs else ''
    _rows = {'ones_row': 1, 'zeros_row': 2}
    CASES += [
        ('g70_s9_iter0' + _t, 70, 9, 21, _rows, dict(n_iterations=0, use_logs=_logs)),
        ('g70_s9_freqs' + _t, 70, 9, 22, _rows, dict(n_iterations=3, use_logs=_logs, freqs=True)),
        ('g70_s9_bounds' + _t, 70, 9, 23, _rows, dict(n_iterations=3, use_logs=_logs, prob_bounds=(0.5, 0.999))),
        ('g70_s9_icp1' + _t, 70, 9, 24, _rows, dict(n_iterations=3, use_logs=_logs, init_capture_prob=1.0)),
        ('g70_s9_float64' + _t, 70, 9, 25, _rows, dict(n_iterations=3, use_logs=_logs, dtype='float64')),
    ]


def main():
    out_dir = os.path.join(HERE, 'bernoulli_cd')
    os.makedirs(out_dir, exist_ok=True)
    worst = 0.0
    for name, G, S, seed, special, args in CASES:
        rng = np.random.default_rng(seed)
        special = {k: v for k, v in special.items() if (v < G if 'row' in k else v < S)}
        X = table(rng, G, S, **special)
        dtype = args.get('dtype', 'int64')
        index = ['gene%d' % i for i in range(G)]
        columns = ['genome%d' % j for j in range(S)]
        df = pd.DataFrame(X.astype(dtype), index=index, columns=columns)
        bounds = args.get('prob_bounds', (0.8, 0.99999999))
        icp = args.get('init_capture_prob', 0.9999)
        freqs = rng.uniform(0.6, 1.05, G) if args.get('freqs') else None       # some outside the bounds, both sides
        logs, n_it = args['use_logs'], args['n_iterations']
        helper = LOGS if logs else PLAIN
        rec = Recorder(getattr(ref_pa, helper), logs)
        setattr(ref_pa, helper, rec)
        buf = io.StringIO()
        try:
            with contextlib.redirect_stdout(buf), warnings.catch_warnings():
                warnings.simplefilter('ignore')
                df_out = ref_pa.compute_bernoulli_grid_core_genome_cd(df, n_iterations=n_it, prob_bounds=bounds,
                                                                      init_capture_prob=icp, init_gene_freqs=freqs,
                                                                      use_logs=logs)
        finally:
            setattr(ref_pa, helper, rec.helper)
        result = df_out.values
        assert np.all(np.isfinite(result)) and len(rec.solves) == n_it * (G + S)
        solves = np.array(rec.solves, dtype=np.float64).reshape(n_it, G + S, 7)
        boundary, trivial = solves[:, :, 4] != 0, solves[:, :, 5] != 0
        with np.errstate(all='ignore'):
            margin = np.minimum(np.abs(solves[:, :, 0]) / solves[:, :, 2], np.abs(solves[:, :, 1]) / solves[:, :, 3])
        margin_a = float(margin[~trivial].min()) if (~trivial).any() else np.inf
        margin_b = float(solves[:, :, 6][boundary].min()) if boundary.any() else np.inf

        start = np.clip(X.sum(1) / float(S) if freqs is None else freqs, bounds[0], bounds[1])
        mine = model.run(X != 0, start, icp, bounds[0], bounds[1], n_it, logs)
        assert not mine.failed.any() and np.array_equal(mine.boundary, boundary)
        diff = float(np.abs(mine.table[1:] - result[1:]).max())
        worst = max(worst, diff)
        assert diff < model.TOL / 10, (name, diff)

        r, c = np.nonzero(X)
        np.savez_compressed(os.path.join(out_dir, name + '.npz'), rows=r.astype(np.int32), cols=c.astype(np.int32),
                            shape=np.array([G, S], dtype=np.int64), index=np.array(index), columns=np.array(columns),
                            dtype=np.array(dtype), n_iterations=np.int64(n_it),
                            prob_bounds=np.array(bounds, dtype=np.float64), init_capture_prob=np.float64(icp),
                            init_gene_freqs=np.zeros(0) if freqs is None else freqs, use_logs=np.bool_(logs),
                            table=result, labels=np.array(df_out.index.tolist()),
                            printed=np.array(buf.getvalue().splitlines()),
                            f_lo=solves[:, :, 0].astype(np.float32), f_hi=solves[:, :, 1].astype(np.float32),
                            scale_lo=solves[:, :, 2].astype(np.float32), scale_hi=solves[:, :, 3].astype(np.float32),
                            boundary=boundary, trivial=trivial)
        print('%-22s %4d x %-3d it %d  (a) %.3g  (b) %.3g  boundary solves %5.1f %%  model - reference %.3g'
              % (name, G, S, n_it, margin_a, margin_b, 100.0 * boundary.mean() if boundary.size else 0.0, diff))
    print('largest model - reference difference over all fixtures: %.3g (tolerance %.3g)' % (worst, model.TOL))


if __name__ == '__main__':
    main()
