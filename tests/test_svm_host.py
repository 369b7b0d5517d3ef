"""Host side of evaluate_model and the bagged linear SVM ensemble (pangenomix_amd/ml_pipelines.py): the
float64 model checks itself against an independent exact solve, the generic (sklearn) path of evaluate_model reproduces
the reference's recorded dictionaries, and the numpy metrics, the vote and the helpers are pinned by fixtures
(tests/golden/make_golden_svm.py). No device is used."""
import contextlib
import io
import json
import os
import sys
import warnings

import numpy as np
import pytest

import svm_fixtures
import svm_model
from pangenomix_amd import _native, ml_pipelines


@pytest.mark.parametrize('name', svm_fixtures.EVAL_CASES)
def test_model_cd_agrees_with_nnls_on_every_fixture_sub_problem(name):
    case = svm_fixtures.eval_case(name)
    fits = svm_fixtures.model_fits(name)
    worst = 0.0
    for (f, e, mask, m), cd in zip(svm_fixtures.sub_problems(case), fits):
        exact = svm_model.fit(case['X'], mask, case['y'], m, svm_fixtures.C, solver='nnls')
        worst = max(worst, np.abs(cd['coef'] - exact['coef']).max(), abs(cd['intercept'] - exact['intercept']))
        assert cd['steps'] > 0
    print('largest |coef(cd) - coef(nnls)| of %s: %.3g' % (name, worst))
    assert worst <= 1e-9


def test_model_cd_keeps_the_pinned_rule_on_a_hand_made_problem():
    """two genomes, one feature each, opposite labels: K = I, Q = [[2 + 1/2C, -1], [-1, 2 + 1/2C]], optimum b = 1 / (1 + 1/2C);
    the first pick is genome 0 (all |PG| tie at 1)."""
    K = np.eye(2, dtype=np.int64)
    beta, steps = svm_model.greedy_cd(K, [1, 0], [1, 1], 1.0, 1e-12)
    assert np.allclose(beta, 1.0 / 1.5, atol=1e-12) and steps > 1
    beta1, steps1 = svm_model.greedy_cd(K, [1, 0], [1, 0], 1.0, 1e-12)         # (only genome 0 is a variable)
    assert steps1 == 1 and beta1[1] == 0.0 and beta1[0] == 1.0 / 2.5


@pytest.mark.parametrize('name', svm_fixtures.EVAL_CASES)
def test_evaluate_model_generic_path_reproduces_the_reference(name):
    pytest.importorskip('sklearn')
    from sklearn.ensemble import BaggingClassifier
    from sklearn.svm import LinearSVC
    case = svm_fixtures.eval_case(name)
    base = BaggingClassifier(LinearSVC(dual=True, random_state=0), n_estimators=7, max_samples=0.8, max_features=0.5,
                             random_state=1)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        got = ml_pipelines.evaluate_model(base, case['lsdf'], case['defs'], case['y_series'], case['known'],
                                          n_folds=case['n_folds'], seed=case['seed'])
    assert sorted(got) == sorted(case['expected'])
    for fold_id, want in case['expected'].items():
        have = dict(got[fold_id])
        assert isinstance(have.pop('Runtime'), float)
        assert list(have) == ['Train_Accuracy', 'Test_Accuracy', 'Train_Precision', 'Test_Precision', 'Train_Recall',
                              'Test_Recall', 'Train_MCC', 'Test_MCC', 'Train_AUC', 'Test_AUC', 'known_AMR_ranks_avg_dense',
                              'known_AMR_blocks']
        have['known_AMR_ranks_avg_dense'] = {k: [float(x) for x in v] for k, v in have['known_AMR_ranks_avg_dense'].items()}
        assert json.loads(json.dumps(have)) == want, fold_id
    strip = lambda text: [ln for ln in text.splitlines() if 'Runtime' not in ln]       # noqa: E731
    assert strip(buf.getvalue()) == strip(case['stdout'])


def test_evaluate_model_takes_explicit_folds_and_needs_no_seed():
    pytest.importorskip('sklearn')
    from sklearn.ensemble import BaggingClassifier
    from sklearn.svm import LinearSVC
    case = svm_fixtures.eval_case('60x90')
    base = BaggingClassifier(LinearSVC(dual=True, random_state=0), n_estimators=7, max_samples=0.8, max_features=0.5,
                             random_state=1)
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        got = ml_pipelines.evaluate_model(base, case['lsdf'], case['defs'], case['y_series'], case['known'], folds=case['folds'])
    for fold_id, want in case['expected'].items():
        assert got[fold_id]['Test_AUC'] == want['Test_AUC'] and got[fold_id]['known_AMR_blocks'] == want['known_AMR_blocks']


def _metrics_cases():
    with open(os.path.join(svm_fixtures.GOLDEN, 'metrics.json')) as fh:
        return json.load(fh)


@pytest.mark.parametrize('case', _metrics_cases(), ids=lambda c: c['name'])
def test_metrics_equal_sklearns_recorded_values(case):
    y, yhat, score = np.array(case['y']), np.array(case['yhat']), np.array(case['score'])
    for module, names in ((svm_model, ('accuracy', 'precision', 'recall', 'mcc', 'auc')),
                          (ml_pipelines, ('_accuracy', '_precision', '_recall', '_mcc', '_roc_auc'))):
        for name in names:
            arg = score if name.endswith('auc') else yhat
            assert float(getattr(module, name)(y, arg)) == case[name.lstrip('_').replace('roc_', '')], name
    assert abs(svm_model.auc_midrank(y, score) - case['auc']) <= 4 * np.finfo(float).eps


def test_auc_on_one_class_raises_and_sir_metrics_use_the_votes():
    with pytest.raises(ValueError, match='Only one class'):
        ml_pipelines._roc_auc([1, 1, 1], [0.1, 0.2, 0.3])

    class Fixed(object):
        def predict(self, X):
            return np.asarray(X)[:, 0]

        def predict_proba(self, X):
            return np.stack([1.0 - np.asarray(X)[:, 1], np.asarray(X)[:, 1]], axis=1)

    X = np.array([[1, 0.9], [0, 0.2], [1, 0.6], [0, 0.6]])
    y = np.array([1, 0, 0, 1])
    got = ml_pipelines.__evaluate_sir_model__(Fixed(), X, y, X[::-1], y[::-1])
    assert got['Train_Accuracy'] == got['Test_Accuracy'] == 0.5 and got['Train_AUC'] == got['Test_AUC'] == 0.875
    assert list(got) == ['Train_Accuracy', 'Test_Accuracy', 'Train_Precision', 'Test_Precision', 'Train_Recall', 'Test_Recall',
                         'Train_MCC', 'Test_MCC', 'Train_AUC', 'Test_AUC']


def test_voting_rule_equals_sklearns_recorded_votes():
    z = np.load(os.path.join(svm_fixtures.GOLDEN, 'voting.npz'))
    assert np.any(z['proba'][:, 0] == 0.5)
    assert np.array_equal(svm_model.vote_proba(z['decisions']), z['proba'])
    assert np.array_equal(svm_model.vote_predict(z['decisions']), z['predict'])
    assert np.array_equal(ml_pipelines.BaggedLinearSVC._votes(z['decisions']), z['proba'])
    tied = z['proba'][:, 0] == 0.5
    assert np.all(z['predict'][tied] == 0)


def test_compute_known_amr_distr_on_hand_made_blocks():
    defs = [['a', 'b'], ['c'], ['d', 'e', 'f'], []]
    counts, blocks = ml_pipelines.compute_known_amr_distr(defs, {'a', 'e', 'f', 'zz'}, selected_blocks=['B2', 'B1', 'B9'])
    assert counts == (4, 2, 2, 1) and blocks == {'B0': ['a'], 'B2': ['e', 'f']}
    assert ml_pipelines.compute_known_amr_distr(defs, set()) == ((0, 0, 0, 0), {})


def test_weight_extraction_averages_over_the_members_that_saw_a_feature():
    class Sub(object):
        def __init__(self, coef):
            self.coef_ = np.array([coef])

    class Ensemble(object):
        estimators_ = [Sub([1.0, 2.0, 0.0]), Sub([3.0, -2.0]), Sub([0.5])]
        estimators_features_ = [np.array([0, 1, 3]), np.array([0, 1]), np.array([2])]

    labels = np.array(['B0', 'B1', 'B2', 'B3'])
    got = ml_pipelines.__extract_weights_from_bagging_ensemble__(Ensemble(), labels)
    assert got.to_dict() == {'B0': 2.0, 'B2': 0.5}                 # B1: mean exactly 0, B3: weight exactly 0 -- dropped
    ranks = ml_pipelines._known_amr_ranks
    with contextlib.redirect_stdout(io.StringIO()):
        out = ranks(got, [['x', 'y'], ['z'], ['w'], ['v']], {'y', 'w', 'v'})
    assert out == {'known_AMR_ranks_avg_dense': {'y': [1.5, 1.0], 'w': [3.0, 2.0]}, 'known_AMR_blocks': {'B0': 1.0, 'B2': 2.0}}


def test_clone_round_trips_the_parameters_and_sklearn_is_imported_lazily():
    import subprocess
    code = 'import sys; import pangenomix_amd.ml_pipelines; sys.exit(int("sklearn" in sys.modules))'
    assert subprocess.call([sys.executable, '-c', code], cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__)))) == 0
    sklearn_base = pytest.importorskip('sklearn.base')
    clf = ml_pipelines.BaggedLinearSVC(n_estimators=50, max_samples=0.8, max_features=0.5, bootstrap=False, C=0.25, tol=1e-8,
                                       max_steps=123, random_state=7)
    twin = sklearn_base.clone(clf)
    assert twin is not clf and twin.get_params() == clf.get_params()
    assert twin.set_params(C=2.0).C == 2.0 and clf.C == 0.25


def test_what_is_not_built_is_refused():
    with pytest.raises(ValueError, match='bootstrap_features'):
        ml_pipelines.BaggedLinearSVC(bootstrap_features=True)
    clf = ml_pipelines.BaggedLinearSVC()
    for params in ({'penalty': 'l1'}, {'loss': 'hinge'}, {'class_weight': 'balanced'}, {'bootstrap_features': True}):
        with pytest.raises(ValueError):
            clf.set_params(**params)
    X = np.array([[1, 0], [0, 1], [1, 1]])
    with pytest.raises(ValueError, match='binary'):
        clf.fit(X * 2, [0, 1, 1])
    with pytest.raises(ValueError, match='two classes'):
        clf.fit(X, [1, 1, 1])
    with pytest.raises(ValueError, match='not fitted'):
        clf.predict(X)


def test_own_draws_follow_the_documented_rule():
    clf = ml_pipelines.BaggedLinearSVC(n_estimators=3, max_samples=0.5, max_features=0.4, random_state=11)
    y = np.array([0, 1] * 10)
    s_sets, f_sets = clf._draw(y, 10)
    rng = np.random.RandomState(11)
    for s, fs in zip(s_sets, f_sets):
        want = rng.randint(0, 20, 10)
        while np.unique(y[want]).size < 2:
            want = rng.randint(0, 20, 10)
        assert np.array_equal(s, want)
        assert np.array_equal(fs, np.sort(rng.permutation(10)[:4]))
    every = ml_pipelines.BaggedLinearSVC(n_estimators=2, bootstrap=False, random_state=0)._draw(y, 10)
    assert all(sorted(s) == list(range(20)) for s in every[0]) and all(list(fs) == list(range(10)) for fs in every[1])


def test_fit_without_a_device_raises():
    import torch
    if torch.cuda.is_available():
        pytest.skip('a GPU is present')
    X = np.array([[1, 0], [0, 1], [1, 1], [0, 0]])
    with pytest.raises(_native.PgxError, match='no usable HIP device|no CPU fallback'):
        ml_pipelines.BaggedLinearSVC(n_estimators=2, random_state=0).fit(X, [0, 1, 1, 0])
