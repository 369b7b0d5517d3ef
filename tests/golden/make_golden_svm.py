#!/usr/bin/env python
"""Golden fixtures for evaluate_model and the bagged linear SVM ensemble (reference ml_pipelines.py evaluate_model and its
helpers), produced by RUNNING THE REFERENCE and sklearn in the build container (needs /root/reference; it
never travels to the GPU box):

    python tests/golden/make_golden_svm.py

The reference's ml_pipelines imports `amr_pangenome.sparse_utils`, a package the reference does not ship: that name is
registered in sys.modules pointing at the reference's own pangenomix.sparse_utils before the import. The reference calls
Series.iteritems(), which pandas 2 no longer has: the name is restored IN THIS SCRIPT ONLY. Only data is written.

tests/golden/svm/eval_<case>.npz   (a) the reference's evaluate_model on a small block x genome case table with
    BaggingClassifier(LinearSVC(dual=True, random_state=0), n_estimators=7, max_samples=0.8, max_features=0.5,
    random_state=1) and an integer seed:
      rows, cols, shape          the table's coordinates (blocks x genomes), labels B<i> / s<j>
      y                          the phenotypes, def_flat / def_off: the features of every block, known: the known AMR set
      seed, n_folds              as handed over
      train_<f>, test_<f>        sklearn's fold indices
      samples [F, E, k], features [F, E, k']   every fitted ensemble's estimators_samples_ / estimators_features_
tests/golden/svm/eval_<case>.json  the returned dictionary without 'Runtime'
tests/golden/svm/metrics.json      (b) sklearn.metrics on hand-made prediction vectors
tests/golden/svm/voting.npz        (c) BaggingClassifier.predict_proba / predict on 6 estimators with tied votes: the
                                   members' decision values, the ensemble's answers

The generator also asserts, with tests/svm_model.py at C = 1 and tol = 1e-10, what tests/test_gpu_svm.py relies on: no
decision of a fixture (a) lies within twice its bound of zero, and no two different |weights| of a fold's features lie
within twice the coefficient bound of each other.
"""
import contextlib
import io
import json
import os
import sys
import types
import warnings

import numpy as np
import pandas as pd
import scipy.sparse

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, '/root/reference')
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import pangenomix.sparse_utils as ref_su      # noqa: E402
_pkg = types.ModuleType('amr_pangenome')
_pkg.sparse_utils = ref_su
sys.modules.setdefault('amr_pangenome', _pkg)
sys.modules.setdefault('amr_pangenome.sparse_utils', ref_su)
import pangenomix.ml_pipelines as ref_ml      # noqa: E402
import sklearn.metrics                         # noqa: E402
from sklearn.ensemble import BaggingClassifier  # noqa: E402
from sklearn.svm import LinearSVC              # noqa: E402

import svm_model                               # noqa: E402

if not hasattr(pd.Series, 'iteritems'):
    pd.Series.iteritems = pd.Series.items

OUT = os.path.join(HERE, 'svm')
FITTED = []


class RecordingBagging(BaggingClassifier):
    def fit(self, X, y, **kw):
        super().fit(X, y, **kw)
        FITTED.append(self)
        return self


def case_table(rng, n_genomes, n_blocks, n_patterns=None):
    """(X bool blocks x genomes, y): a few blocks carry the phenotype, the rest is noise; with n_patterns the genomes are
    copies of that many patterns (heavily duplicated genomes, some with opposite phenotypes)."""
    n_distinct = n_patterns or n_genomes
    X = rng.random((n_blocks, n_distinct)) < rng.beta(0.7, 2.0, n_blocks)[:, None]
    score = X[:5].sum(axis=0) - X[5:9].sum(axis=0) + rng.normal(0, 0.8, n_distinct)
    y = (score > np.median(score)).astype(int)
    if n_patterns:
        pick = rng.integers(0, n_patterns, n_genomes)
        X, y = X[:, pick], y[pick]
        flip = rng.random(n_genomes) < 0.08
        y = np.where(flip, 1 - y, y)
    X[0, :] |= ~X.any(axis=0)                                  # (no genome without a block, no block without a genome)
    for r in np.flatnonzero(~X.any(axis=1)):
        X[r, rng.integers(0, X.shape[1])] = True
    return X, y


def model_margins(name, X, y, folds, samples, features):
    """the two assertions of the module docstring, on the float64 model"""
    G = X.T                                                     # genomes x blocks
    for f, (train, test) in enumerate(folds):
        weights = {}
        for e in range(samples.shape[1]):
            mask = np.zeros(G.shape[1], dtype=bool)
            mask[features[f, e]] = True
            m = svm_model.multiplicities(train[samples[f, e]], G.shape[0])
            fit = svm_model.fit(G, mask, y, m, 1.0, 1e-10)
            db = svm_model.decision_bound(1.0, m, 1e-10, int(mask.sum()))
            assert np.abs(fit['decision']).min() > 2 * db, (name, f, e, np.abs(fit['decision']).min(), db)
            for r in features[f, e]:
                weights.setdefault(int(r), []).append(fit['coef'][r])
            cb = svm_model.coef_bound(1.0, m, 1e-10)
        w = np.sort(np.abs(np.array([np.mean(v) for v in weights.values()])))
        gaps = np.diff(w)
        assert not np.any((gaps > 0) & (gaps <= 2 * cb)), (name, f, gaps[gaps > 0].min(), cb)


def eval_case(name, rng, n_genomes, n_blocks, seed, n_patterns=None):
    X, y = case_table(rng, n_genomes, n_blocks, n_patterns)
    rows, cols = np.nonzero(X)
    index = ['B%d' % i for i in range(n_blocks)]
    columns = ['s%d' % j for j in range(n_genomes)]
    coo = scipy.sparse.coo_matrix((np.ones(rows.size, dtype=np.int64), (rows, cols)), shape=X.shape)
    lsdf = ref_su.LightSparseDataFrame(index, columns, coo)
    sizes = rng.integers(1, 4, n_blocks)
    defs = [np.array(['g%d_%d' % (i, k) for k in range(sizes[i])]) for i in range(n_blocks)]
    flat = np.concatenate(defs)
    known = sorted(set(flat[rng.random(flat.size) < 0.08]) | {defs[0][0], defs[6][0]})
    y_series = pd.Series(y.astype(float), index=columns)
    base = RecordingBagging(LinearSVC(dual=True, random_state=0), n_estimators=7, max_samples=0.8, max_features=0.5,
                            random_state=1)
    del FITTED[:]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        out = ref_ml.evaluate_model(base, lsdf, defs, y_series, set(known), n_folds=5, seed=seed)
    import sklearn.model_selection
    skf = sklearn.model_selection.StratifiedKFold(n_splits=5, shuffle=True, random_state=seed)
    folds = list(skf.split(coo.T.tocsr(), y))
    assert len(FITTED) == 5
    samples = np.array([[np.asarray(s) for s in clf.estimators_samples_] for clf in FITTED])
    features = np.array([[np.asarray(s) for s in clf.estimators_features_] for clf in FITTED])
    model_margins(name, X, y, folds, samples, features)
    for fold in out.values():
        del fold['Runtime']
        fold['known_AMR_ranks_avg_dense'] = {k: [float(x) for x in v] for k, v in fold['known_AMR_ranks_avg_dense'].items()}
        for k in list(fold):
            if not isinstance(fold[k], dict):
                fold[k] = float(fold[k])
    arrays = {'rows': rows.astype(np.uint16), 'cols': cols.astype(np.uint16), 'shape': np.array(X.shape, dtype=np.int64),
              'y': y.astype(np.int8), 'def_flat': flat, 'def_off': np.r_[0, np.cumsum(sizes)].astype(np.int64),
              'known': np.array(known), 'seed': np.int64(seed), 'n_folds': np.int64(5),
              'samples': samples.astype(np.uint16), 'features': features.astype(np.uint16),
              'stdout': np.array(buf.getvalue())}
    for f, (train, test) in enumerate(folds):
        arrays['train_%d' % f] = train.astype(np.uint16)
        arrays['test_%d' % f] = test.astype(np.uint16)
    path = os.path.join(OUT, 'eval_%s.npz' % name)
    np.savez_compressed(path, **arrays)
    with open(os.path.join(OUT, 'eval_%s.json' % name), 'w') as fh:
        json.dump(out, fh, indent=0, sort_keys=True)
    print('%s: %s, %d bytes, test AUCs %s' % (name, X.shape, os.path.getsize(path),
                                              [round(out[k]['Test_AUC'], 3) for k in sorted(out)]))


def metrics_cases():
    rng = np.random.default_rng(5)
    cases = []

    def add(name, y, yhat, score):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            cases.append({'name': name, 'y': [int(v) for v in y], 'yhat': [int(v) for v in yhat],
                          'score': [float(v) for v in score],
                          'accuracy': float(sklearn.metrics.accuracy_score(y, yhat)),
                          'precision': float(sklearn.metrics.precision_score(y, yhat)),
                          'recall': float(sklearn.metrics.recall_score(y, yhat)),
                          'mcc': float(sklearn.metrics.matthews_corrcoef(y, yhat)),
                          'auc': float(sklearn.metrics.roc_auc_score(y, score))})

    y = np.array([0, 0, 1, 1, 1, 0, 1, 0, 0, 1])
    add('perfect', y, y, y / 1.0)
    add('no_positive_predictions', y, np.zeros(10, dtype=int), np.zeros(10))
    add('all_positive_predictions', y, np.ones(10, dtype=int), np.ones(10))
    add('inverted', y, 1 - y, 1.0 - y)
    add('tied_scores', y, [0, 1, 1, 0, 1, 0, 1, 1, 0, 0], np.array([1, 3, 3, 2, 5, 0, 4, 3, 2, 2]) / 7.0)
    for k in range(12):
        n = int(rng.integers(5, 80))
        yy = rng.integers(0, 2, n)
        yy[:2] = [0, 1]
        votes = rng.integers(0, 8, n)
        add('random_%d' % k, yy, (votes > 3).astype(int), votes / 7.0)
    with open(os.path.join(OUT, 'metrics.json'), 'w') as fh:
        json.dump(cases, fh, indent=0)
    print('metrics: %d cases' % len(cases))


def voting_case():
    rng = np.random.default_rng(8)
    X = (rng.random((40, 30)) < 0.3).astype(float)
    y = (X[:, 0] + X[:, 1] - X[:, 2] + rng.normal(0, 0.7, 40) > 0.3).astype(int)
    clf = BaggingClassifier(LinearSVC(dual=True, random_state=0, C=0.01), n_estimators=6, max_samples=0.5, max_features=0.3,
                            random_state=3).fit(X, y)
    decisions = np.array([est.decision_function(X[:, fs]) for est, fs in zip(clf.estimators_, clf.estimators_features_)])
    proba, pred = clf.predict_proba(X), clf.predict(X)
    assert np.any(proba[:, 0] == 0.5), 'no tied vote in the fixture'
    assert np.abs(decisions).min() > 1e-9
    np.savez_compressed(os.path.join(OUT, 'voting.npz'), decisions=decisions, proba=proba, predict=pred.astype(np.int8))
    print('voting: %d tied votes of %d' % (np.sum(proba[:, 0] == 0.5), pred.size))


def main():
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(61)
    eval_case('60x90', rng, 60, 90, seed=3)
    eval_case('130x300', rng, 130, 300, seed=4)
    eval_case('duplicated_genomes', rng, 100, 120, seed=5, n_patterns=14)
    metrics_cases()
    voting_case()


if __name__ == '__main__':
    main()
