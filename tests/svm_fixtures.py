"""TEST INFRASTRUCTURE: the fixtures of tests/golden/svm (make_golden_svm.py) as objects, and the float64 model's answer
for them, computed once per process and shared (never modified) by the tests that need it."""
import functools
import json
import os

import numpy as np
import pandas as pd
import scipy.sparse

import svm_model
from pangenomix_amd import sparse_utils

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'svm')
EVAL_CASES = ('60x90', '130x300', 'duplicated_genomes')
C, TOL = 1.0, 1e-10                 # what the class-level tests fit with (make_golden_svm.py checked the margins for these)


@functools.lru_cache(maxsize=None)
def eval_case(name):
    z = np.load(os.path.join(GOLDEN, 'eval_%s.npz' % name))
    n_blocks, n_genomes = (int(v) for v in z['shape'])
    rows, cols = z['rows'].astype(np.int64), z['cols'].astype(np.int64)
    coo = scipy.sparse.coo_matrix((np.ones(rows.size, dtype=np.int64), (rows, cols)), shape=(n_blocks, n_genomes))
    lsdf = sparse_utils.LightSparseDataFrame(['B%d' % i for i in range(n_blocks)], ['s%d' % j for j in range(n_genomes)], coo)
    off = z['def_off']
    defs = [z['def_flat'][off[i]:off[i + 1]] for i in range(n_blocks)]
    y = z['y'].astype(int)
    n_folds = int(z['n_folds'])
    with open(os.path.join(GOLDEN, 'eval_%s.json' % name)) as fh:
        expected = json.load(fh)
    return {'name': name, 'lsdf': lsdf, 'defs': defs, 'known': set(z['known'].tolist()), 'y': y,
            'y_series': pd.Series(y.astype(float), index=lsdf.columns), 'seed': int(z['seed']), 'n_folds': n_folds,
            'folds': [(z['train_%d' % f].astype(np.int64), z['test_%d' % f].astype(np.int64)) for f in range(n_folds)],
            'samples': z['samples'].astype(np.int64), 'features': z['features'].astype(np.int64), 'expected': expected,
            'X': np.asarray(coo.todense(), dtype=bool).T, 'stdout': str(z['stdout'])}


def sub_problems(case):
    """[(fold, estimator, mask bool [n_blocks], multiplicities [n_genomes])] in the order fit_many lays them out"""
    n_genomes, n_blocks = case['X'].shape
    out = []
    for f, (train, _) in enumerate(case['folds']):
        for e in range(case['samples'].shape[1]):
            mask = np.zeros(n_blocks, dtype=bool)
            mask[case['features'][f, e]] = True
            out.append((f, e, mask, svm_model.multiplicities(train[case['samples'][f, e]], n_genomes)))
    return out


@functools.lru_cache(maxsize=None)
def model_fits(name):
    """the model's fit of every sub-problem of a case at (C, TOL), in sub_problems() order"""
    case = eval_case(name)
    return [svm_model.fit(case['X'], mask, case['y'], m, C, TOL) for _, _, mask, m in sub_problems(case)]
