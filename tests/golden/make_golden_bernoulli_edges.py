#!/usr/bin/env python
"""Golden fixtures of compute_bernoulli_grid_core_genome on tables without, or almost without, absent cells (pan-genome
tables of a clonal species look like that), produced by RUNNING THE REFERENCE with its default arguments in the build
container (needs /root/reference; it never travels to the GPU box):

    python tests/golden/make_golden_bernoulli_edges.py

tests/golden/bernoulli_edges/<case>.npz has the fields of tests/golden/core/<case>.npz (make_golden_core.py, whose
helpers this uses). They are kept out of core/ because on such tables the reference's sum of log(fl(p q)) and the
device's rowsum log p + colsum log q differ by more than the rtol 1e-12 that the tests over core/ apply: see
tests/bernoulli_model.py for the bound that holds.
"""
import contextlib
import io
import os
import warnings

import numpy as np
import pandas as pd

from make_golden_core import HERE, ref_grad, ref_ll, ref_pa, scales

G, S = 128, 12
CASES = [('g128_s12_all_ones', []), ('g128_s12_three_zeros', [(0, 0), (77, 5), (127, 11)])]


def main():
    out = os.path.join(HERE, 'bernoulli_edges')
    os.makedirs(out, exist_ok=True)
    for k, (name, zeros) in enumerate(CASES):
        rng = np.random.default_rng(100 + k)
        X = np.ones((G, S), dtype=np.int64)
        for i, j in zeros:
            X[i, j] = 0
        index = ['gene%d' % i for i in range(G)]
        columns = ['genome%d' % j for j in range(S)]
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf), warnings.catch_warnings():
            warnings.simplefilter('ignore')
            df_opt, res = ref_pa.compute_bernoulli_grid_core_genome(pd.DataFrame(X, index=index, columns=columns))
        lo, hi = 0.8, 0.99999999                             # the reference's default prob_bounds
        edges = rng.uniform(lo, hi, G + S)
        edges[::3], edges[1::3] = lo, hi
        points = np.stack([df_opt['initial'].values[1:], np.asarray(res.x),
                           rng.uniform(lo, lo + 0.999 * (hi - lo), G + S), edges])
        with warnings.catch_warnings(), np.errstate(all='ignore'):
            warnings.simplefilter('ignore')
            lls = [ref_ll(X, pt[:G], pt[G:]) for pt in points]
            grads = [ref_grad(X, pt[:G], pt[G:]) for pt in points]
        gscale, llscale = zip(*(scales(X, pt[:G], pt[G:]) for pt in points))
        r, c = np.nonzero(X)
        np.savez_compressed(os.path.join(out, name + '.npz'), rows=r.astype(np.int32), cols=c.astype(np.int32),
                            shape=np.array([G, S], dtype=np.int64), index=np.array(index), columns=np.array(columns),
                            prob_bounds=np.array((lo, hi)), init_capture_prob=np.float64(0.9999),
                            init_gene_freqs=np.zeros(0), labels=np.array(df_opt.index.tolist()),
                            initial=df_opt['initial'].values, optimum=df_opt['optimum'].values, x=np.asarray(res.x),
                            fun=np.float64(res.fun), nit=np.int64(res.nit), nfev=np.int64(res.nfev),
                            status=np.int64(res.status), printed=np.array(buf.getvalue().splitlines()), points=points,
                            point_ll=np.array(lls), point_grad=np.array(grads), point_scale=np.array(gscale),
                            point_ll_scale=np.array(llscale))
        print('%s: LL %r -> %r nit %d nfev %d status %d' % (name, df_opt['initial'].values[0], -res.fun, res.nit,
                                                           res.nfev, res.status))


if __name__ == '__main__':
    main()
