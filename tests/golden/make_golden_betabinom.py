#!/usr/bin/env python
"""Golden fixtures for compute_beta_binomial_core_genome, ks_montecarlo_bbn and draw_bbn (reference
pangenome_analysis.py:295-400, :457-509), produced by RUNNING THE REFERENCE in the build container (needs
/root/reference; it never travels to the GPU box):

    python tests/golden/make_golden_betabinom.py

`pangenome_analysis` imports statsmodels.stats at module level and its beta-binomial estimator calls
statsmodels.stats.stattools.durbin_watson. statsmodels is not installed, so a placeholder module is registered whose
durbin_watson is sum(diff(r)**2) / sum(r**2). The fixtures' Durbin-Watson values are therefore pinned to that
restatement, not to statsmodels itself.

For every case, tests/golden/betabinom/<case>.npz holds
  kind                        'table' (a binary table), 'counts' (a df_counts Series), 'ks' (a direct ks_montecarlo_bbn
                              call) or 'draws' (a direct draw_bbn call)
  seed, start_pos             np.random.seed(seed) before the call (then the state's pos set to start_pos, if >= 0)
  rows, cols, shape, index, columns    table cases: the table's COO coordinates (int32), shape and labels
  freq_index, freq_values     table cases: the reference's frequency Series (Counter of row sums, in its order)
  counts_index, counts_values counts cases: the df_counts Series passed
  frac_recovered, num_points, list_mode, ks_iter       the arguments (num_points as a list; list_mode: passed as one)
  result_index, result_columns, result                 the returned Series (result_columns empty) or DataFrame
  y_index, y_values, n, a, b, iterations, sim_limit    ks cases: the arguments; pvalue, ks_stat, ks_sim: the results
  n, a, b, size, sim_limit, draws                      draws cases
  key, pos                    the generator state after the call
  error_type, error_message   where the reference raised ('' otherwise)
  n_ks, ks<k>_*               every ks_montecarlo_bbn call the reference made inside compute_beta_binomial_core_genome,
                              in order: its arguments (y_index, y_values, n, a, b, iterations, sim_limit), the generator
                              state before it (key_before, pos_before), its results (pvalue, ks_stat, ks_sim) and the
                              state after it (key_after, pos_after)
"""
import collections
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, '/root/reference')
sys.path.insert(0, '/root/reference/pangenomix')


def _durbin_watson(resids):
    resids = np.asarray(resids)
    return np.sum(np.diff(resids) ** 2) / np.sum(resids ** 2)


for _name in ('statsmodels', 'statsmodels.stats', 'statsmodels.stats.stattools'):
    sys.modules.setdefault(_name, types.ModuleType(_name))
sys.modules['statsmodels'].stats = sys.modules['statsmodels.stats']
sys.modules['statsmodels.stats'].stattools = sys.modules['statsmodels.stats.stattools']
sys.modules['statsmodels.stats.stattools'].durbin_watson = _durbin_watson

import pandas as pd                                       # noqa: E402
import scipy.sparse                                       # noqa: E402
import pangenomix.pangenome_analysis as ref_pa            # noqa: E402
import pangenomix.sparse_utils as ref_su                  # noqa: E402

OUT = os.path.join(HERE, 'betabinom')


def gene_counts(rng, n_genomes, n_core, n_acc, a, b):
    """Genomes per gene: core genes missing from BetaBinomial(n_genomes, a, b) genomes, accessory genes uniform."""
    misses = rng.binomial(n_genomes, rng.beta(a, b, n_core))
    core = n_genomes - misses
    acc = rng.integers(1, n_genomes, n_acc)
    return np.concatenate((acc, core))


def table_of(rng, counts, n_genomes):
    """A binary table whose row g is present in counts[g] random genomes."""
    rows, cols = [], []
    for g, c in enumerate(counts):
        cols.append(np.sort(rng.choice(n_genomes, size=int(c), replace=False)))
        rows.append(np.full(int(c), g))
    return np.concatenate(rows).astype(np.int32), np.concatenate(cols).astype(np.int32)


def ascending_series(counts):
    """a df_counts Series {genomes: genes} in ascending order of genomes (as from a table sorted by frequency)"""
    vals, tally = np.unique(counts, return_counts=True)
    return pd.Series(tally.astype(np.int64), index=vals.astype(np.int64))


class KsRecorder(object):
    """Stands in for the reference's ks_montecarlo_bbn (looked up by name at call time) and records every call."""

    def __init__(self):
        self.real = ref_pa.ks_montecarlo_bbn
        self.calls = []

    def __call__(self, Ycounts, n, a, b, iterations=100, sim_limit=1000):
        st = np.random.get_state()
        rec = {'y_index': np.asarray(Ycounts.index, dtype=np.int64), 'y_values': np.asarray(Ycounts.values),
               'n': np.int64(n), 'a': np.float64(a), 'b': np.float64(b), 'iterations': np.int64(iterations),
               'sim_limit': np.int64(sim_limit), 'key_before': st[1].copy(), 'pos_before': np.int64(st[2])}
        pvalue, ks_stat, ks_sim = self.real(Ycounts, n, a, b, iterations=iterations, sim_limit=sim_limit)
        st = np.random.get_state()
        rec.update(pvalue=np.float64(pvalue), ks_stat=np.float64(ks_stat), ks_sim=np.asarray(ks_sim),
                   key_after=st[1].copy(), pos_after=np.int64(st[2]))
        self.calls.append(rec)
        return pvalue, ks_stat, ks_sim


def seed(s, start_pos=-1):
    np.random.seed(s)
    if start_pos >= 0:
        st = np.random.get_state()
        np.random.set_state(('MT19937', st[1], start_pos))


def run(fn, *args, **kwargs):
    """(result, error_type, error_message) of fn(*args, **kwargs), warnings silenced"""
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        try:
            return fn(*args, **kwargs), '', ''
        except Exception as e:                      # noqa: BLE001 (the reference's exception is the fixture)
            return None, type(e).__name__, str(e)


def save(name, **arrays):
    st = np.random.get_state()
    np.savez_compressed(os.path.join(OUT, name + '.npz'), key=st[1], pos=np.int64(st[2]), **arrays)


def estimator_case(name, s, frac_recovered=0.999, num_points=100, ks_iter=1000, table=None, counts=None):
    """compute_beta_binomial_core_genome on a table (rows, cols, shape) or a counts Series"""
    rec = KsRecorder()
    ref_pa.ks_montecarlo_bbn = rec
    try:
        if table is not None:
            rows, cols, shape = table
            index = ['gene%d' % i for i in range(shape[0])]
            columns = ['genome%d' % j for j in range(shape[1])]
            m = scipy.sparse.coo_matrix((np.ones(rows.size, dtype=np.int64), (rows, cols)), shape=shape)
            frame = ref_su.LightSparseDataFrame(index, columns, m).to_sparse_arrays()
            gene_mat = ref_su.sparse_arrays_to_spmatrix(frame)
            freq = pd.Series(collections.Counter(np.array(gene_mat.sum(axis=1))[:, 0]))
            extra = dict(kind=np.array('table'), rows=rows, cols=cols, shape=np.array(shape, dtype=np.int64),
                         index=np.array(index), columns=np.array(columns),
                         freq_index=np.asarray(freq.index, dtype=np.int64), freq_values=np.asarray(freq.values))
            seed(s)
            res, et, em = run(ref_pa.compute_beta_binomial_core_genome, frame, frac_recovered=frac_recovered,
                              num_points=num_points, ks_iter=ks_iter)
        else:
            extra = dict(kind=np.array('counts'), counts_index=np.asarray(counts.index, dtype=np.int64),
                         counts_values=np.asarray(counts.values))
            seed(s)
            res, et, em = run(ref_pa.compute_beta_binomial_core_genome, None, frac_recovered=frac_recovered,
                              df_counts=counts, num_points=num_points, ks_iter=ks_iter)
    finally:
        ref_pa.ks_montecarlo_bbn = rec.real
    if res is None:
        r_index, r_columns, r_values = np.zeros(0, dtype='U1'), np.zeros(0, dtype='U1'), np.zeros(0)
    elif isinstance(res, pd.DataFrame):
        r_index, r_columns, r_values = np.asarray(res.index, dtype=np.int64), np.array(list(res.columns)), res.values
    else:
        r_index, r_columns, r_values = np.array(list(res.index)), np.zeros(0, dtype='U1'), res.values
    ks = {}
    for k, call in enumerate(rec.calls):
        ks.update({'ks%d_%s' % (k, key): v for key, v in call.items()})
    list_mode = type(num_points) != int
    save(name, seed=np.int64(s), start_pos=np.int64(-1), frac_recovered=np.float64(frac_recovered),
         num_points=np.array(num_points if list_mode else [num_points], dtype=np.int64), list_mode=np.bool_(list_mode),
         ks_iter=np.int64(ks_iter), result_index=r_index, result_columns=r_columns,
         result=np.asarray(r_values, dtype=np.float64), error_type=np.array(et), error_message=np.array(em),
         n_ks=np.int64(len(rec.calls)), **extra, **ks)
    print('%s: %s %s ks calls %d sim_limits %s result %s' % (name, et or 'ok', em[:60], len(rec.calls),
                                                            [int(c['sim_limit']) for c in rec.calls],
                                                            '' if res is None else np.asarray(r_values).ravel()[:7]))


def ks_case(name, s, y, n, a, b, iterations, sim_limit, start_pos=-1):
    seed(s, start_pos)
    res, et, em = run(ref_pa.ks_montecarlo_bbn, y, n, a, b, iterations=iterations, sim_limit=sim_limit)
    pvalue, ks_stat, ks_sim = res if res is not None else (np.nan, np.nan, np.zeros(0))
    save(name, kind=np.array('ks'), seed=np.int64(s), start_pos=np.int64(start_pos),
         y_index=np.asarray(y.index, dtype=np.int64), y_values=np.asarray(y.values), n=np.int64(n), a=np.float64(a),
         b=np.float64(b), iterations=np.int64(iterations), sim_limit=np.int64(sim_limit), pvalue=np.float64(pvalue),
         ks_stat=np.float64(ks_stat), ks_sim=np.asarray(ks_sim, dtype=np.float64), error_type=np.array(et),
         error_message=np.array(em))
    print('%s: %s %s pvalue %r' % (name, et or 'ok', em[:60], pvalue))


def draws_case(name, s, n, a, b, size, sim_limit):
    seed(s)
    res, et, em = run(ref_pa.draw_bbn, n, a, b, size, sim_limit=sim_limit)
    save(name, kind=np.array('draws'), seed=np.int64(s), start_pos=np.int64(-1), n=np.int64(n), a=np.float64(a),
         b=np.float64(b), size=np.int64(size), sim_limit=np.int64(sim_limit),
         draws=np.zeros(0, dtype=np.int64) if res is None else np.asarray(res), error_type=np.array(et),
         error_message=np.array(em))
    print('%s: %s %s' % (name, et or 'ok', em[:60]))


def main():
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(11)
    # a small table, rows in ascending frequency (a sensible fit), and the same table with its rows scrambled
    S = 60
    counts = np.sort(gene_counts(rng, S, 280, 20, 0.6, 40.0))
    rows, cols = table_of(rng, counts, S)
    estimator_case('table_ascending', 101, num_points=8, ks_iter=300, table=(rows, cols, (counts.size, S)))
    perm = rng.permutation(counts.size)
    estimator_case('table_scrambled', 102, num_points=8, ks_iter=300,
                   table=(perm[rows].astype(np.int32), cols, (counts.size, S)))
    # counts Series at 400 genomes (about 3,400 genes in the fitted points)
    c400 = ascending_series(gene_counts(rng, 400, 3400, 600, 0.5, 60.0))
    estimator_case('counts_400', 103, num_points=100, ks_iter=500, counts=c400)
    estimator_case('counts_400_list', 104, num_points=[30, 60, 100], ks_iter=200, counts=c400)
    estimator_case('counts_400_frac1', 105, frac_recovered=1.0, num_points=100, ks_iter=100, counts=c400)
    # nearly every gene in every genome: sim_limit == 0 (nan p-value, nothing drawn)
    estimator_case('counts_sim_limit_0', 106, num_points=3, ks_iter=100,
                   counts=pd.Series([2, 1, 10 ** 12], index=[398, 399, 400]))
    # large: 4,000 genomes, 12,000 genes (10,482 in the fitted points), 2,000 iterations
    c4000 = ascending_series(gene_counts(rng, 4000, 11000, 1000, 0.8, 40.0))
    estimator_case('counts_4000', 107, num_points=250, ks_iter=2000, counts=c4000)
    # sim_limit above the LDS path's limit (4,096 values)
    c20000 = ascending_series(gene_counts(rng, 20000, 8000, 0, 3.0, 60.0))
    estimator_case('counts_20000', 108, num_points=1500, ks_iter=40, counts=c20000)

    # direct calls
    y = pd.Series([5, 40, 300], index=[2, 1, 0])
    ks_case('ks_small', 201, y, 60, 0.4, 30.0, 500, 40)
    ks_case('ks_miss_beyond_limit', 202, pd.Series([5, 40, 300], index=[12, 1, 0]), 60, 0.4, 30.0, 50, 10)
    ks_case('ks_sim_limit_0', 203, y, 60, 0.4, 30.0, 50, 0)
    far = pd.Series([3, 9, 20], index=[900, 30, 5])
    ks_case('ks_lds_edge_4096', 204, far, 6000, 0.9, 6.0, 60, 4096)
    ks_case('ks_global_4097', 205, far, 6000, 0.9, 6.0, 60, 4097)
    ks_case('ks_one_iteration', 206, pd.Series([1], index=[3]), 60, 0.4, 30.0, 1, 40)
    ks_case('ks_pos_623', 207, y, 60, 0.4, 30.0, 7, 40, start_pos=623)
    draws_case('draws_small', 301, 60, 0.4, 30.0, 1001, 40)
    draws_case('draws_empty_range', 302, 60, 0.4, 30.0, 5, 0)


if __name__ == '__main__':
    main()
