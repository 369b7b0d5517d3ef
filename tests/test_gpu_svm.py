"""The bagged linear SVM ensemble on the device (pangenomix_amd/csrc/svm.hip) through the C ABI, against the
float64 model (tests/svm_model.py) at TWICE the derived bounds: with n the drawn genomes of a sub-problem,
    |beta, coef, intercept - model's| <= 2 * (2 C max(m) n tol),     |decision - model's| <= 2 * (|mask| + 1) (2 C max(m) n tol)
(the device and the model each lie within one bound of the unique optimum). Then the class and evaluate_model on the
fixtures of tests/golden/svm, whose margins make votes, metrics and ranks exact."""
import contextlib
import io

import numpy as np
import pytest

import svm_fixtures
import svm_model
from pangenomix_amd import _native, ml_pipelines

pytestmark = pytest.mark.gpu

OUTPUTS = ('beta', 'coef', 'intercept', 'decision', 'steps')


def stride_of(n_rows):
    return int(_native.lib().pgx_bitmap_stride_words(int(n_rows)))


def pack_masks(masks, n_rows):
    bits = np.zeros((len(masks), stride_of(n_rows) * 64), dtype=bool)
    bits[:, :n_rows] = np.asarray(masks, dtype=bool)
    return np.packbits(bits, axis=1, bitorder='little').view('<u8').astype(np.uint64)


def run(ctx, X, masks, problems, y, tol=1e-10, max_steps=0):
    """X bool [n_genomes, n_rows]; masks: bool [n_masks, n_rows]; problems: [(mask index, C, multiplicities)]"""
    n, n_rows = X.shape
    genomes, rows = np.nonzero(X)
    return ctx.svm_bag(rows, genomes, n_rows, n, pack_masks(masks, n_rows), [p[0] for p in problems],
                       [p[1] for p in problems], np.array([p[2] for p in problems]), np.asarray(y, dtype=np.uint8), tol=tol,
                       max_steps=max_steps)


def check(out, X, masks, problems, y, tol, what, max_steps=None):
    """every output of every sub-problem against the model at twice the bounds; returns the largest differences"""
    worst = {'coef': 0.0, 'decision': 0.0}
    for p, (t, C, m) in enumerate(problems):
        mask = np.asarray(masks[t], dtype=bool)
        want = svm_model.fit(X, mask, y, m, C, tol)
        cb = 2 * svm_model.coef_bound(C, m, tol)
        db = 2 * svm_model.decision_bound(C, m, tol, int(mask.sum()))
        d = {k: float(np.abs(out[k][p] - want[k]).max()) for k in ('beta', 'coef', 'intercept', 'decision')}
        print('%s p=%d steps %d (model %d) |d beta| %.3g |d coef| %.3g |d icpt| %.3g (bound %.3g) |d dec| %.3g (bound %.3g)'
              % (what, p, out['steps'][p], want['steps'], d['beta'], d['coef'], d['intercept'], cb, d['decision'], db))
        assert d['beta'] <= cb and d['coef'] <= cb and d['intercept'] <= cb and d['decision'] <= db, (what, p, d, cb, db)
        assert np.all(out['beta'][p][np.asarray(m) == 0] == 0.0) and np.all(out['beta'][p] >= 0.0), (what, p)
        assert np.all(out['coef'][p][~mask] == 0.0), (what, p)
        assert 0 < out['steps'][p] <= (max_steps or 1000000 + 2000 * X.shape[0]), (what, p)
        worst = {k: max(worst[k], d[k]) for k in worst}
    return worst


def two_classes(rng, n):
    y = (rng.random(n) < 0.5).astype(np.uint8)
    y[0], y[1] = 1, 0
    return y


def draw(rng, y, share=0.8):
    """multiplicities of a bootstrap sample of a training set of `share` of the genomes; both classes drawn"""
    n = y.size
    while True:
        train = np.sort(rng.permutation(n)[:max(2, int(share * n))])
        m = np.bincount(train[rng.integers(0, train.size, train.size)], minlength=n)
        if np.unique(y[m > 0]).size == 2:
            return m


def random_case(seed, n, n_rows, n_problems, density=0.2, share=0.8):
    rng = np.random.default_rng(seed)
    X = rng.random((n, n_rows)) < density
    y = two_classes(rng, n)
    masks, problems = [], []
    for p in range(n_problems):
        mask = rng.random(n_rows) < 0.5
        mask[rng.integers(0, n_rows)] = True
        masks.append(mask)
        problems.append((p, 1.0, draw(rng, y, share) if n > 2 else np.ones(n, dtype=np.int64)))
    return X, y, masks, problems


@pytest.mark.parametrize('n,n_rows,n_problems', [(2, 1, 1), (3, 63, 2), (63, 64, 2), (64, 65, 1), (65, 1023, 2), (129, 1024, 2),
                                                 (257, 1025, 2), (400, 1025, 2), (65, 129, 35)])
def test_shapes_against_the_model(gpu_ctx, n, n_rows, n_problems):
    X, y, masks, problems = random_case(100 + n, n, n_rows, n_problems)
    out = run(gpu_ctx, X, masks, problems, y)
    check(out, X, masks, problems, y, 1e-10, 'n=%d rows=%d' % (n, n_rows))


@pytest.mark.parametrize('n_rows', [65, 1024, 1025])
def test_masks_one_feature_every_feature_and_the_last_valid_bit(gpu_ctx, n_rows):
    rng = np.random.default_rng(n_rows)
    n = 66
    X = rng.random((n, n_rows)) < 0.3
    X[::2, n_rows - 1] = True
    X[:, 3] = rng.random(n) < 0.5
    y = two_classes(rng, n)
    one, last = np.zeros(n_rows, dtype=bool), np.zeros(n_rows, dtype=bool)
    one[3], last[n_rows - 1] = True, True
    masks = [one, np.ones(n_rows, dtype=bool), last]
    problems = [(t, 1.0, draw(rng, y)) for t in range(3)]
    out = run(gpu_ctx, X, masks, problems, y)
    check(out, X, masks, problems, y, 1e-10, 'masks rows=%d' % n_rows)
    # bits of a mask behind n_rows are ignored (the bitmap's pad bits are zero)
    packed = pack_masks(masks, n_rows)
    packed[:, (n_rows + 63) // 64:] = np.uint64(0xFFFFFFFFFFFFFFFF)
    genomes, rows = np.nonzero(X)
    again = gpu_ctx.svm_bag(rows, genomes, n_rows, n, packed, [0, 1, 2], [1.0] * 3, np.array([p[2] for p in problems]), y)
    for k in OUTPUTS:
        assert again[k].tobytes() == out[k].tobytes(), k


def test_shared_and_private_masks_give_identical_outputs(gpu_ctx):
    X, y, masks, problems = random_case(7, 129, 300, 4)
    shared = [(0, 1.0, m) for _, _, m in problems]
    a = run(gpu_ctx, X, masks[:1], shared, y)
    b = run(gpu_ctx, X, [masks[0]] * 4, [(p, 1.0, m) for p, (_, _, m) in enumerate(problems)], y)
    for k in OUTPUTS:
        assert a[k].tobytes() == b[k].tobytes(), k
    check(a, X, masks[:1], shared, y, 1e-10, 'shared mask')


def test_data_edges(gpu_ctx):
    rng = np.random.default_rng(21)
    n, n_rows = 70, 130
    X = rng.random((n, n_rows)) < 0.25
    y = two_classes(rng, n)
    mask = rng.random(n_rows) < 0.5
    X[5, mask] = False                                  # a genome with no feature in the mask
    X[9] = X[8]                                         # two identical genomes with opposite labels
    y[8], y[9] = 1, 0
    m = np.ones(n, dtype=np.int64)
    out = run(gpu_ctx, X, [mask], [(0, 1.0, m)], y)
    check(out, X, [mask], [(0, 1.0, m)], y, 1e-10, 'no feature / identical genomes')
    # a training set that leaves genomes out: their beta is 0, their decision is still right (checked against the model)
    m_out = m.copy()
    m_out[40:] = 0
    out = run(gpu_ctx, X, [mask], [(0, 1.0, m_out)], y)
    check(out, X, [mask], [(0, 1.0, m_out)], y, 1e-10, 'genomes left out')
    assert np.all(out['beta'][0][40:] == 0.0) and np.all(out['decision'][0][40:] != 0.0)


def test_multiplicities_equal_explicitly_duplicated_rows(gpu_ctx):
    rng = np.random.default_rng(22)
    n, n_rows, C, tol = 65, 90, 1.0, 1e-10
    X = rng.random((n, n_rows)) < 0.25
    y = two_classes(rng, n)
    mask = rng.random(n_rows) < 0.6
    m = rng.choice([0, 1, 7], size=n)
    m[0], m[1], m[2] = 7, 1, 0
    out = run(gpu_ctx, X, [mask], [(0, C, m)], y, tol)
    rep = np.repeat(np.arange(n), m)
    want = svm_model.fit(X[rep], mask, y[rep], np.ones(rep.size, dtype=np.int64), C, tol)
    beta_sum = np.bincount(rep, weights=want['beta'], minlength=n)
    bound = svm_model.coef_bound(C, m, tol) + svm_model.coef_bound(C, np.ones(rep.size), tol)
    dec = X[:, mask].astype(float) @ want['coef'][mask] + want['intercept']
    d = (np.abs(out['beta'][0] - beta_sum).max(), np.abs(out['coef'][0] - want['coef']).max(),
         abs(out['intercept'][0] - want['intercept']), np.abs(out['decision'][0] - dec).max())
    print('duplicated rows: differences %s, bound %.3g' % (d, bound))
    assert max(d[:3]) <= bound and d[3] <= (mask.sum() + 1) * bound
    assert {0, 1, 7} == set(m.tolist())


@pytest.mark.parametrize('C', [1e-3, 1.0, 1e3])
@pytest.mark.parametrize('tol', [1e-6, 1e-12])
def test_c_and_tol(gpu_ctx, C, tol):
    X, y, masks, problems = random_case(31, 65, 129, 2)
    problems = [(t, C, m) for t, _, m in problems]
    out = run(gpu_ctx, X, masks, problems, y, tol)
    check(out, X, masks, problems, y, tol, 'C=%g tol=%g' % (C, tol))


def test_capacity_limit(gpu_ctx):
    """PGX_SVM_MAX_GENOMES genomes (the solver's largest LDS image) with a small training set; one more is refused."""
    rng = np.random.default_rng(41)
    n, n_rows = _native.Context.SVM_MAX_GENOMES, 64
    X = rng.random((n, n_rows)) < 0.3
    y = two_classes(rng, n)
    m = np.zeros(n, dtype=np.int64)
    m[rng.permutation(n)[:100]] = 1
    m[0] = m[1] = 1
    mask = np.ones(n_rows, dtype=bool)
    out = run(gpu_ctx, X, [mask], [(0, 1.0, m)], y)
    check(out, X, [mask], [(0, 1.0, m)], y, 1e-10, 'n=%d' % n)
    Xb = np.vstack([X, X[:1]])
    with pytest.raises(_native.PgxError) as e:
        run(gpu_ctx, Xb, [mask], [(0, 1.0, np.r_[m, 0])], np.r_[y, 0])
    assert e.value.status == -5
    assert gpu_ctx.svm_bag_workspace_bytes(n_rows, n + 1, 1) == 0


def test_error_paths(gpu_ctx):
    X, y, masks, problems = random_case(51, 40, 70, 2)
    m = problems[0][2]
    bad = []
    one_class = np.where(y == 1, m + 1, 0)
    bad.append(('one class', lambda: run(gpu_ctx, X, masks, [(0, 1.0, one_class)], y)))
    bad.append(('empty mask', lambda: run(gpu_ctx, X, [masks[0], np.zeros(70, dtype=bool)], problems, y)))
    bad.append(('mask index', lambda: run(gpu_ctx, X, masks, [(2, 1.0, m)], y)))
    bad.append(('mask index', lambda: run(gpu_ctx, X, masks, [(-1, 1.0, m)], y)))
    for C in (0.0, -1.0, float('nan'), float('inf')):
        bad.append(('C', lambda C=C: run(gpu_ctx, X, masks, [(0, C, m)], y)))
    for tol in (0.0, float('nan'), float('inf')):
        bad.append(('tol', lambda tol=tol: run(gpu_ctx, X, masks, problems, y, tol)))
    bad.append(('label', lambda: run(gpu_ctx, X, masks, problems, np.where(np.arange(40) == 7, 2, y))))
    genomes, rows = np.nonzero(X)
    packed = pack_masks(masks, 70)
    mult = np.array([p[2] for p in problems])
    bad.append(('duplicate', lambda: gpu_ctx.svm_bag(np.r_[rows, rows[:1]], np.r_[genomes, genomes[:1]], 70, 40, packed, [0, 1],
                                                     [1.0, 1.0], mult, y)))
    bad.append(('out of range', lambda: gpu_ctx.svm_bag(np.r_[rows, 70], np.r_[genomes, 0], 70, 40, packed, [0, 1], [1.0, 1.0],
                                                        mult, y)))
    for what, call in bad:
        with pytest.raises(_native.PgxError) as e:
            call()
        assert e.value.status == -1, (what, str(e.value))
    with pytest.raises(_native.PgxError) as e:               # a run that ends normally and says so
        run(gpu_ctx, X, masks, problems, y, max_steps=1)
    assert e.value.status == -6 and 'steps' in str(e.value)
    out = run(gpu_ctx, X, masks, problems, y)                # the context is as good as before
    check(out, X, masks, problems, y, 1e-10, 'after the errors')


def test_three_calls_give_equal_bytes(gpu_ctx):
    X, y, masks, problems = random_case(100 + 400, 400, 1025, 2)
    first = run(gpu_ctx, X, masks, problems, y)
    for _ in range(2):
        again = run(gpu_ctx, X, masks, problems, y)
        for k in OUTPUTS:
            assert again[k].tobytes() == first[k].tobytes(), k


def test_device_pointer_entry_equals_the_host_entry(gpu_ctx):
    """pgx_svm_bag_dev on caller tensors -- results and a workspace of exactly the size asked for between guard bands, full
    of garbage, inputs made on the caller's stream (tests/dev_entry_checks.py) -- gives the bytes of pgx_svm_bag, on the
    null stream and on a side stream; the inputs are not written; a broken sub-problem is reported from the device."""
    import dev_entry_checks as chk
    X, y, masks, problems = random_case(61, 130, 300, 3)
    n, n_rows = X.shape
    P = len(problems)
    want = run(gpu_ctx, X, masks, problems, y)
    genomes, rows = np.nonzero(X)
    bits = gpu_ctx.presence_bitmap(rows, genomes, n_rows, n)
    packed = pack_masks(masks, n_rows)
    mask_of = np.array([p[0] for p in problems], dtype=np.int32)
    Cs = np.array([p[1] for p in problems], dtype=np.float64)
    mult = np.array([p[2] for p in problems], dtype=np.uint16)
    nws = gpu_ctx.svm_bag_workspace_bytes(n_rows, n, len(masks))
    assert nws >= len(masks) * n * n * 4
    sizes = {'beta': P * n * 8, 'coef': P * n_rows * 8, 'intercept': P * 8, 'decision': P * n * 8, 'steps': P * 4}
    results = []
    for kind, fill in zip(chk.STREAMS, chk.FILLS):
        with chk.stream_scope(kind) as st:
            ws = chk.guarded(nws, fill)
            outs = {k: chk.guarded(b, fill) for k, b in sizes.items()}
            ups = [chk.upload(a) for a in (bits, packed, mask_of, Cs, mult, y)]
            with chk.unchanged(*ups):
                gpu_ctx.svm_bag_dev(ups[0].ptr, n_rows, n, ups[1].ptr, len(masks), ups[2].ptr, ups[3].ptr, ups[4].ptr, P,
                                    ups[5].ptr, outs['beta'].ptr, outs['coef'].ptr, outs['intercept'].ptr, outs['decision'].ptr,
                                    outs['steps'].ptr, ws.ptr, nws, stream=st)
        for b in [ws] + list(outs.values()):
            b.assert_guards_intact()
        results.append(tuple(outs[k].numpy(np.uint32 if k == 'steps' else np.float64) for k in OUTPUTS))
    got = chk.same_bytes(results)
    for g, k in zip(got, OUTPUTS):
        assert g.tobytes() == want[k].tobytes(), k
    with chk.stream_scope('null') as st:
        ws = chk.guarded(nws, 0x5A)
        outs = {k: chk.guarded(b, 0x5A) for k, b in sizes.items()}
        bad_of = mask_of.copy()
        bad_of[1] = len(masks)
        ups = [chk.upload(a) for a in (bits, packed, bad_of, Cs, mult, y)]
        args = lambda nbytes: (ups[0].ptr, n_rows, n, ups[1].ptr, len(masks), ups[2].ptr, ups[3].ptr, ups[4].ptr, P,   # noqa: E731
                               ups[5].ptr, outs['beta'].ptr, outs['coef'].ptr, outs['intercept'].ptr, outs['decision'].ptr,
                               outs['steps'].ptr, ws.ptr, nbytes)
        with pytest.raises(_native.PgxError, match='workspace too small'):
            gpu_ctx.svm_bag_dev(*args(nws - 1), stream=st)
        with pytest.raises(_native.PgxError, match='mask index out of range') as e:
            gpu_ctx.svm_bag_dev(*args(nws), stream=st)
        assert e.value.status == -1
    for b in [ws] + list(outs.values()):
        b.assert_guards_intact()


# -- the class and evaluate_model on the fixtures ---------------------------------------------------------------------------
def fit_folds(ctx, case, many=True):
    clf = ml_pipelines.BaggedLinearSVC(n_estimators=7, max_samples=0.8, max_features=0.5, C=svm_fixtures.C, tol=svm_fixtures.TOL,
                                       ctx=ctx)
    X = case['lsdf'].data.T.tocsr()
    trains = [train for train, _ in case['folds']]
    return X, clf.fit_many(X, case['y'], trains, case['samples'], case['features'])


@pytest.mark.parametrize('name', svm_fixtures.EVAL_CASES)
def test_class_equals_the_model_on_the_recorded_draws(gpu_ctx, name):
    case = svm_fixtures.eval_case(name)
    fits = svm_fixtures.model_fits(name)
    subs = svm_fixtures.sub_problems(case)
    # the fixture's margins: no decision within twice its bound of zero, so every vote is decided
    for (f, e, mask, m), fit in zip(subs, fits):
        assert np.abs(fit['decision']).min() > 2 * svm_model.decision_bound(svm_fixtures.C, m, svm_fixtures.TOL, int(mask.sum()))
    X, fitted = fit_folds(gpu_ctx, case)
    n_est = case['samples'].shape[1]
    worst = 0.0
    for f, clf in enumerate(fitted):
        mine = fits[f * n_est:(f + 1) * n_est]
        for e, (est, fit) in enumerate(zip(clf.estimators_, mine)):
            _, _, mask, m = subs[f * n_est + e]
            cb = 2 * svm_model.coef_bound(svm_fixtures.C, m, svm_fixtures.TOL)
            features = case['features'][f, e]                    # (in the order they were drawn: coef_ follows it)
            assert est.coef_.shape == (1, features.size) and np.array_equal(clf.estimators_features_[e], features)
            assert np.array_equal(clf.estimators_samples_[e], case['samples'][f, e])
            d = max(np.abs(est.coef_[0] - fit['coef'][features]).max(), abs(est.intercept_[0] - fit['intercept']))
            worst = max(worst, d)
            assert d <= cb
        decisions = np.array([fit['decision'] for fit in mine])
        assert np.array_equal(clf.predict_proba(X), svm_model.vote_proba(decisions))           # on EVERY sample
        assert np.array_equal(clf.predict(X), svm_model.vote_predict(decisions))
        assert np.array_equal(clf.classes_, [0, 1]) and clf.n_steps_.shape == (n_est,)
        # another table (here: a copy) is multiplied out on the host and votes the same
        assert np.array_equal(clf.predict(X.copy()), clf.predict(X))
    print('%s: largest |coef - model| %.3g' % (name, worst))


def test_fit_many_equals_fit_fold_by_fold(gpu_ctx):
    case = svm_fixtures.eval_case('60x90')
    X, fitted = fit_folds(gpu_ctx, case)
    for f, (train, _) in enumerate(case['folds']):
        single = ml_pipelines.BaggedLinearSVC(n_estimators=7, C=svm_fixtures.C, tol=svm_fixtures.TOL, ctx=gpu_ctx)
        single.fit(X[train, :], case['y'][train], case['samples'][f], case['features'][f])
        for a, b in zip(single.estimators_, fitted[f].estimators_):
            assert a.coef_.tobytes() == b.coef_.tobytes() and a.intercept_.tobytes() == b.intercept_.tobytes()
        assert np.array_equal(single.n_steps_, fitted[f].n_steps_)
        assert single.decision_function_all(X[train, :]) is not None


def test_own_draws_fit_and_are_reproducible(gpu_ctx):
    case = svm_fixtures.eval_case('60x90')
    X = case['lsdf'].data.T.tocsr()
    a = ml_pipelines.BaggedLinearSVC(n_estimators=4, max_samples=0.8, max_features=0.5, random_state=5, ctx=gpu_ctx).fit(X, case['y'])
    b = ml_pipelines.BaggedLinearSVC(n_estimators=4, max_samples=0.8, max_features=0.5, random_state=5, ctx=gpu_ctx).fit(X, case['y'])
    assert all(x.coef_.tobytes() == z.coef_.tobytes() for x, z in zip(a.estimators_, b.estimators_))
    assert a.predict(X).shape == (60,) and np.mean(a.predict(X) == case['y']) > 0.7


@pytest.mark.parametrize('name', svm_fixtures.EVAL_CASES)
def test_evaluate_model_on_the_device_equals_the_model(gpu_ctx, name):
    case = svm_fixtures.eval_case(name)
    fits = svm_fixtures.model_fits(name)
    subs = svm_fixtures.sub_problems(case)
    n_est = case['samples'].shape[1]

    class Recorded(ml_pipelines.BaggedLinearSVC):
        """the fixture's draws instead of the class's own"""

        def fit_many(self, X, y, train_sets, sample_sets=None, feature_sets=None):
            return ml_pipelines.BaggedLinearSVC.fit_many(self, X, y, train_sets, case['samples'], case['features'])

    base = Recorded(n_estimators=n_est, max_samples=0.8, max_features=0.5, C=svm_fixtures.C, tol=svm_fixtures.TOL)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        got = ml_pipelines.evaluate_model(base, case['lsdf'], case['defs'], case['y_series'], case['known'], folds=case['folds'],
                                          ctx=gpu_ctx)
    assert buf.getvalue().count('FOLD:') == 5 and 'Training model...' in buf.getvalue()
    y = case['y']
    for f, (train, test) in enumerate(case['folds']):
        mine = fits[f * n_est:(f + 1) * n_est]
        have = got['FOLD%d' % (f + 1)]
        decisions = np.array([fit['decision'] for fit in mine])
        proba, pred = svm_model.vote_proba(decisions), svm_model.vote_predict(decisions)
        for part, idx in (('Train', train), ('Test', test)):
            for key, fn in (('Accuracy', svm_model.accuracy), ('Precision', svm_model.precision), ('Recall', svm_model.recall),
                            ('MCC', svm_model.mcc)):
                assert have['%s_%s' % (part, key)] == fn(y[idx], pred[idx]), (f, part, key)
            assert have['%s_AUC' % part] == svm_model.auc(y[idx], proba[idx, 1]), (f, part)
        assert have['Runtime'] > 0

        # the model's ensemble through the package's host helpers: the ranks are equal because no two different |weights|
        # of the fold lie within twice the coefficient bound of each other (asserted here, and by the generator)
        class Model(object):
            estimators_ = [ml_pipelines._SubClassifier(fit['coef'][fs], fit['intercept'])
                           for fit, fs in zip(mine, case['features'][f])]
            estimators_features_ = list(case['features'][f])

        weights = ml_pipelines.__extract_weights_from_bagging_ensemble__(Model, case['lsdf'].index)
        cb = max(svm_model.coef_bound(svm_fixtures.C, m, svm_fixtures.TOL) for _, _, _, m in subs[f * n_est:(f + 1) * n_est])
        gaps = np.diff(np.sort(np.abs(weights.values)))
        assert not np.any((gaps > 0) & (gaps <= 2 * cb)), 'the fixture has two |weights| closer than twice the bound'
        with contextlib.redirect_stdout(io.StringIO()):
            want = ml_pipelines._known_amr_ranks(weights, case['defs'], case['known'])
        assert have['known_AMR_ranks_avg_dense'] == want['known_AMR_ranks_avg_dense'], f
        assert have['known_AMR_blocks'] == want['known_AMR_blocks'], f
        assert len(want['known_AMR_blocks']) > 0
