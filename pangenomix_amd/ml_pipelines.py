"""
The per-phenotype association screen on MI355X.

Mirror of the part of the reference's ml_pipelines.py that consumes the feature x genome table before any model is
trained: `prepare_amr_case_data` (pick the genomes that have a phenotype for a drug, drop the features that are now
empty, merge features with identical occurrence into blocks), `contingency_tables_from_sparse` (TP / FP / FN / TN of
every feature against a phenotype vector), `adjusted_lor` and `prefilter_features_by_lor`. Same names, positional order
and defaults; `ctx` is the only addition.

All of it is integer work on the genome-major bitmap libpgx builds and keeps resident (pangenomix_amd/csrc/assoc.hip,
DESIGN.md 6d): the rows' bits among the selected genomes, AND + popcount against the phenotype masks, equality of rows.
The device returns integers; the float columns of the contingency table and the one log2 are formed on the host with
the reference's expressions. The reference densifies the table in batches. There is no CPU fallback.

The model half: `evaluate_model` (stratified cross-validation of a bagging ensemble, metrics, weights, ranks of the
known AMR genes), its helpers and `compute_known_amr_distr`, with `BaggedLinearSVC` as the device classifier: the whole
cross-validation -- n_folds x n_estimators linear SVMs in their duals on the bitmap's AND + popcount Gram matrix -- is
ONE library call (pangenomix_amd/csrc/svm.hip). Any sklearn classifier is still accepted and goes fold by
fold as in the reference; sklearn is imported inside the functions that need it, never when this module is imported.
"""

from __future__ import print_function

import time

import numpy as np

from . import sparse_utils


def _target_masks(targets):
    """uint64 [n_targets, ceil(n_samples / 64) or 1]: bit j of row t = targets[t, j] is non-zero (np.logical_and's
    reading of a number: a NaN counts)."""
    n_targets, n_samples = targets.shape
    words = max(1, (n_samples + 63) // 64)
    bits = np.zeros((n_targets, words * 64), dtype=bool)
    bits[:, :n_samples] = targets != 0
    return np.packbits(bits, axis=1, bitorder='little').view('<u8').astype(np.uint64, copy=False)


def contingency_tables_from_sparse(sp_features, target, batch_size=10000, ctx=None):
    """Contingency tables between every feature (row) of a binary feature x sample table and a target vector.

    sp_features : scipy.sparse matrix, dense 2-D array of 0/1 or LightSparseDataFrame (never densified)
    target      : one value per sample; a sample counts as positive where the value is non-zero (a NaN too). A 2-D
                  array (n_targets, n_samples) screens all its rows in ONE pass over the table.
    batch_size  : accepted for compatibility and ignored
    ctx         : optional pangenomix_amd._native.Context (default: process-wide)

    Returns float64 (n_features, 4): TP, FP, FN, TN per feature -- TP and the features' incidence are counted on the device,
    FP = incidence - TP, FN = target.sum() - TP, TN = n_samples - TP - FP - FN as the reference forms them -- or
    (n_targets, n_features, 4), whose row t equals the call with target[t].
    """
    who = 'contingency_tables_from_sparse'
    table = sparse_utils._screen_table(sp_features, who)
    n_features, n_samples = table[2]
    target = np.asarray(target)
    targets = target[None, :] if target.ndim == 1 else target
    if targets.ndim != 2 or targets.shape[1] != n_samples:
        raise ValueError('target must hold one value per sample')
    out = sparse_utils._screen(table, who, ctx, masks=_target_masks(targets))
    incidence = out['incidence'].astype(np.int64)
    contingency = np.zeros((targets.shape[0], n_features, 4))
    for t in range(targets.shape[0]):
        positives = float(targets[t].sum())
        TPs = out['tp'][t].astype(np.int64)
        FPs = incidence - TPs
        FNs = positives - TPs
        TNs = n_samples - TPs - FPs - FNs
        contingency[t, :, 0] = TPs
        contingency[t, :, 1] = FPs
        contingency[t, :, 2] = FNs
        contingency[t, :, 3] = TNs
    return contingency[0] if target.ndim == 1 else contingency


def adjusted_lor(contingency):
    """Adjusted log2 odds ratio of every row of a contingency table (TP, FP, FN, TN), as defined in
    https://doi.org/10.1371/journal.pcbi.1007608: each cell is offset by the positive / negative rate."""
    TPs, FPs = contingency[:, 0], contingency[:, 1]
    FNs, TNs = contingency[:, 2], contingency[:, 3]
    PRs = np.divide(TPs + FNs, contingency.sum(axis=1, dtype='float'))
    NRs = 1.0 - PRs
    numerator = np.multiply(TPs + PRs, TNs + NRs)
    denominator = np.multiply(FPs + NRs, FNs + PRs)
    return np.log2(np.divide(numerator, denominator))


def _select_by_lor(lors, max_features):
    """Row positions kept by the LOR filter: half = max_features // 2; the rows ordered by LOR descending with a STABLE
    sort (equal LORs keep ascending position, NaN last); the first `half` of that order, then its last `half`."""
    order = np.argsort(-np.asarray(lors, dtype=np.float64), kind='stable')
    half = int(max_features) // 2
    return order[:half].tolist() + order[order.size - half:].tolist()


def prefilter_features_by_lor(lsdf_case_block, df_amr_org_drug, min_freq=3, max_features=10000, ctx=None):
    """Filter compressed features by raw frequency and LOR: with 10000 features allowed, the 5000 with the highest and the
    5000 with the lowest LOR are kept.

    lsdf_case_block : LightSparseDataFrame, block x genome table from prepare_amr_case_data()
    df_amr_org_drug : pd.Series, phenotypes by genome from prepare_amr_case_data()
    min_freq        : minimum occurrence of a feature (default 3; 0 = no frequency filter)
    max_features    : maximum number of features returned (default 10000)

    The selection among more than max_features rows is this package's own rule (_select_by_lor): the
    reference's line raises TypeError under Python 3, and its unstable sort leaves the order of equal LORs open.
    """
    if min_freq > 0:
        feature_freqs = np.array(lsdf_case_block.data.sum(axis=1))[:, 0]
        count_filtered = np.where(feature_freqs >= min_freq)[0]
        lsdf = lsdf_case_block.islice(i_indices=count_filtered)
    else:
        lsdf = lsdf_case_block
    if lsdf.shape[0] <= max_features:
        return lsdf
    contingency = contingency_tables_from_sparse(lsdf.data, df_amr_org_drug.values.astype(float), batch_size=10000, ctx=ctx)
    lors = adjusted_lor(contingency)
    lsdf_case_block2 = lsdf.islice(i_indices=_select_by_lor(lors, max_features))
    print('Species x drug LOR-selected compressed features:', lsdf_case_block2.shape)
    return lsdf_case_block2


def prepare_amr_case_data(drug, lsdf_features, df_amr_org, df_known_amr, ctx=None):
    """The data of one species x drug case: the drug's phenotypes (genomes without one dropped), the known AMR features
    of the drug, the feature table reduced to those genomes and to the features that occur in them, and that table with
    features of identical occurrence merged into blocks.

    drug          : name of the antimicrobial (a column of df_amr_org and df_known_amr)
    lsdf_features : LightSparseDataFrame, feature x genome table
    df_amr_org    : pd.DataFrame, genome x drug phenotypes (NaN = none)
    df_known_amr  : pd.DataFrame, feature x drug table of known AMR features

    Returns (df_amr_org_drug, known_amr_drug_set, lsdf_case_features, lsdf_case_block, case_block_defs);
    case_block_defs[i] = the labels of the features in block i. For the gene table returned by build_cds_pangenome()
    the column selection, the empty-row drop and the blocks come from ONE pass over the bitmap the pipeline left on
    the device (nothing of the table is uploaded).
    """
    who = 'prepare_amr_case_data'
    df_amr_org_drug = df_amr_org.loc[:, drug].dropna()
    print('Species x drug AMR data:', df_amr_org_drug.shape)
    df_known_amr_drug = df_known_amr.loc[:, drug].dropna()
    known_amr_drug_set = set(df_known_amr_drug.index)
    print('Species x drug AMR features:', len(known_amr_drug_set))

    table = sparse_utils._screen_table(lsdf_features, who)
    if table[3] is not None and table[2][0] > 0 and len(df_amr_org_drug) > 0:
        i_columns = [lsdf_features.column_map[x] for x in df_amr_org_drug.keys()]
        out = sparse_utils._screen(table, who, ctx, col_map=i_columns, blocks=True, drop_empty=True)
        kept = np.where(out['incidence'] > 0)[0]
        # labelslice + drop_empty in one: columns by CSC, kept rows by CSR (the matrices the two calls would build)
        case = lsdf_features.data.tocsc()[:, i_columns].tocsr()[kept, :]
        lsdf_case_features = sparse_utils.LightSparseDataFrame(lsdf_features.index[kept], lsdf_features.columns[i_columns], case)
        print('Species x drug reduced features:', lsdf_case_features.shape)
        position = np.cumsum(out['incidence'] > 0) - 1        # a kept row's position in the reduced table
        lsdf_case_block, case_block_defs = sparse_utils._block_frame(lsdf_case_features, out['block_of_row'][kept],
                                                                     position[out['rep_row']], case)
    else:
        lsdf_case_features = lsdf_features.labelslice(columns=df_amr_org_drug.keys())
        lsdf_case_features = lsdf_case_features.drop_empty(axis='index')
        print('Species x drug reduced features:', lsdf_case_features.shape)
        lsdf_case_block, case_block_defs = sparse_utils.compress_rows(lsdf_case_features, ctx=ctx)
    print('Species x drug compressed features:', lsdf_case_block.shape)
    return df_amr_org_drug, known_amr_drug_set, lsdf_case_features, lsdf_case_block, case_block_defs


# -- the model half: evaluate_model on a bagged ensemble of linear SVMs ------------------------------------
class _SubClassifier(object):
    """One fitted member of a BaggedLinearSVC: coef_ (1, n_selected) over its own features, intercept_ (1,)."""

    def __init__(self, coef, intercept):
        self.coef_ = np.asarray(coef, dtype=np.float64).reshape(1, -1)
        self.intercept_ = np.array([intercept], dtype=np.float64)


class BaggedLinearSVC(object):
    """Bagging ensemble of linear SVMs -- sklearn's BaggingClassifier(LinearSVC(penalty='l2', loss='squared_hinge',
    dual=True, C=C)) -- trained on the device: every member is solved in its dual by the pinned greedy coordinate descent
    of pgx.h (pgx_svm_bag), all members of a call (of all folds with fit_many) at once. There is no CPU fallback.

    n_estimators, max_samples, max_features, bootstrap : as sklearn's BaggingClassifier (a float is a share, an int a count)
    bootstrap_features : must be False (a feature drawn twice is not a mask)
    C         : the members' C
    tol       : largest |projected gradient| of the dual at the end; every coefficient is then within
                2 C max(multiplicity) n_samples tol of the optimum's
    max_steps : coordinate steps allowed per member (None: the library's 1,000,000 + 2,000 n_samples); more raise PgxError
    random_state : seed of the draws, see below
    ctx       : optional pangenomix_amd._native.Context (default: process-wide)

    Only the l2 penalty with the squared hinge loss, without class weights, is built: set_params refuses anything else.

    The draws (this package's own rule; NOT sklearn's random stream, whose draws can be reproduced by handing its
    estimators_samples_ / estimators_features_ to fit as sample_sets / feature_sets): rng =
    numpy.random.RandomState(random_state); for member 0, 1, ... in turn, first the samples -- rng.randint(0, n, k) with
    bootstrap, else the first k of rng.permutation(n), k = max_samples or int(max_samples * n), at least 1; drawn again,
    at most 100 times, while they carry one class only -- then the features: all of them in order when k' = max_features
    or int(max_features * n_features) (at least 1) is n_features, else the first k' of rng.permutation(n_features),
    sorted. fit_many starts every training set from a fresh RandomState(random_state), as cloning does.

    After fit: estimators_ (coef_, intercept_), estimators_features_, estimators_samples_, classes_, n_steps_.
    """

    _PARAMS = ('n_estimators', 'max_samples', 'max_features', 'bootstrap', 'bootstrap_features', 'C', 'tol', 'max_steps',
               'random_state', 'ctx')

    def __init__(self, n_estimators=10, max_samples=1.0, max_features=1.0, bootstrap=True, bootstrap_features=False, C=1.0,
                 tol=1e-10, max_steps=None, random_state=None, ctx=None):
        if bootstrap_features:
            raise ValueError('BaggedLinearSVC: bootstrap_features=True is not supported (a feature drawn twice is not a mask)')
        self.n_estimators = n_estimators
        self.max_samples = max_samples
        self.max_features = max_features
        self.bootstrap = bootstrap
        self.bootstrap_features = bootstrap_features
        self.C = C
        self.tol = tol
        self.max_steps = max_steps
        self.random_state = random_state
        self.ctx = ctx

    # sklearn's estimator protocol (sklearn.base.clone needs no more)
    def get_params(self, deep=True):
        return {name: getattr(self, name) for name in self._PARAMS}

    def set_params(self, **params):
        for name, value in params.items():
            if name not in self._PARAMS:
                raise ValueError('BaggedLinearSVC has no parameter %r: only the l2 penalty with the squared hinge loss, '
                                 'without class weights, is built' % name)
            if name == 'bootstrap_features' and value:
                raise ValueError('BaggedLinearSVC: bootstrap_features=True is not supported')
            setattr(self, name, value)
        return self

    def __sklearn_clone__(self):
        return type(self)(**self.get_params())               # (ctx is shared, not copied)

    @staticmethod
    def _count(share, n, what):
        k = int(share) if isinstance(share, (int, np.integer)) and not isinstance(share, bool) else int(share * n)
        if not 1 <= max(k, 1) <= n:
            raise ValueError('%s must select between 1 and %d' % (what, n))
        return max(k, 1)

    def _draw(self, y_train, n_features):
        """(sample_sets, feature_sets) of one training set by the rule of the class docstring"""
        rng = np.random.RandomState(self.random_state)
        n = y_train.size
        k = self._count(self.max_samples, n, 'max_samples')
        kf = self._count(self.max_features, n_features, 'max_features')
        sample_sets, feature_sets = [], []
        for _ in range(int(self.n_estimators)):
            for attempt in range(100):
                draw = rng.randint(0, n, k) if self.bootstrap else rng.permutation(n)[:k]
                if np.unique(y_train[draw]).size == 2:
                    break
            else:
                raise ValueError('BaggedLinearSVC: 100 draws of %d samples carried one class only' % k)
            sample_sets.append(draw)
            feature_sets.append(np.arange(n_features) if kf == n_features else np.sort(rng.permutation(n_features)[:kf]))
        return sample_sets, feature_sets

    def fit(self, X, y, sample_sets=None, feature_sets=None):
        """X: genomes x features, binary -- dense, scipy.sparse or the transposed matrix of a LightSparseDataFrame (stored
        values other than 1 and duplicate coordinates raise ValueError). sample_sets / feature_sets: one list of sample
        positions (repeats = bootstrap copies) / of distinct feature positions per member, instead of this class's draws."""
        n = X.shape[0]
        fitted = self.fit_many(X, y, [np.arange(n)], None if sample_sets is None else [sample_sets],
                               None if feature_sets is None else [feature_sets])[0]
        self.__dict__.update({k: v for k, v in fitted.__dict__.items() if k not in self._PARAMS})
        return self

    def fit_many(self, X, y, train_sets, sample_sets=None, feature_sets=None):
        """One ensemble per training set (row positions of X), all in ONE library call; returns the fitted classifiers,
        each a clone of this one. sample_sets[f][e] / feature_sets[f][e]: the explicit draws of member e of training set f
        (sample positions WITHIN the training set, as sklearn's estimators_samples_ are). Each classifier remembers the
        decisions of every row of X, so predicting on X (the same object) or on rows of it costs nothing more."""
        from . import _native
        who = 'BaggedLinearSVC.fit'
        table = sparse_utils._screen_table(X.T, who)
        rows, cols, (n_features, n), _ = table
        y = np.asarray(y)
        if y.shape != (n,):
            raise ValueError('y must hold one label per row of X')
        classes = np.unique(y)
        if classes.size != 2:
            raise ValueError('BaggedLinearSVC needs exactly two classes')
        labels = (y == classes[1]).astype(np.uint8)
        if n == 0 or n_features == 0:
            raise ValueError('BaggedLinearSVC needs a table with samples and features')
        if not (self.C > 0 and np.isfinite(self.C) and self.tol > 0 and np.isfinite(self.tol)):
            raise ValueError('C and tol must be finite and positive')
        n_est = int(self.n_estimators)
        plans = []
        for f, train in enumerate(train_sets):
            train = np.asarray(train, dtype=np.int64)
            if sample_sets is None or feature_sets is None:
                own_s, own_f = self._draw(labels[train], n_features)
            s_sets = own_s if sample_sets is None else [np.asarray(s, dtype=np.int64) for s in sample_sets[f]]
            f_sets = own_f if feature_sets is None else [np.asarray(s, dtype=np.int64) for s in feature_sets[f]]
            if len(s_sets) != n_est or len(f_sets) != n_est:
                raise ValueError('one sample set and one feature set per estimator')
            plans.append((train, s_sets, f_sets))
        stride = int(_native.lib().pgx_bitmap_stride_words(n_features))
        mask_index, mask_rows, mask_of, mult = {}, [], [], []
        for train, s_sets, f_sets in plans:
            for s, fs in zip(s_sets, f_sets):
                if fs.size == 0 or fs.min() < 0 or fs.max() >= n_features or np.unique(fs).size != fs.size:
                    raise ValueError('a feature set must hold distinct positions of features')
                if s.size == 0 or s.min() < 0 or s.max() >= train.size:
                    raise ValueError('a sample set must hold positions of the training set')
                bits = np.zeros(stride * 64, dtype=bool)
                bits[fs] = True
                key = bits.tobytes()
                if key not in mask_index:
                    mask_index[key] = len(mask_rows)
                    mask_rows.append(np.packbits(bits, bitorder='little').view('<u8'))
                mask_of.append(mask_index[key])
                m = np.bincount(train[s], minlength=n)
                if m.max() > 65535:
                    raise ValueError('a sample drawn more than 65535 times')
                mult.append(m.astype(np.uint16))
        ctx = self.ctx or _native.default_context()
        t0 = time.time()
        try:
            out = ctx.svm_bag(rows, cols, n_features, n, np.array(mask_rows, dtype=np.uint64), mask_of,
                              np.full(len(mask_of), float(self.C)), np.array(mult), labels, tol=float(self.tol),
                              max_steps=int(self.max_steps or 0))
        except _native.PgxError as e:
            if getattr(e, 'status', 0) == -1 and 'duplicate' in str(e):
                raise ValueError(who + ' needs a table without duplicate entries')
            raise
        call_seconds = time.time() - t0
        fitted = []
        for f, (train, s_sets, f_sets) in enumerate(plans):
            clf = BaggedLinearSVC(**self.get_params())
            sl = slice(f * n_est, (f + 1) * n_est)
            clf.classes_ = classes
            clf.estimators_features_ = f_sets
            clf.estimators_samples_ = s_sets
            clf.estimators_ = [_SubClassifier(out['coef'][p][fs], out['intercept'][p])
                               for p, fs in zip(range(sl.start, sl.stop), f_sets)]
            clf.n_steps_ = out['steps'][sl].copy()
            clf.n_features_in_ = n_features
            clf.call_seconds_ = call_seconds
            clf._train_index = train
            clf._table = X
            clf._table_decisions = out['decision'][sl]        # [n_estimators, rows of X]
            fitted.append(clf)
        return fitted

    def _check_fitted(self):
        if not hasattr(self, 'estimators_'):
            raise ValueError('this BaggedLinearSVC is not fitted yet')

    def decision_function_all(self, X):
        """(n_estimators, n_samples): every member's decision value of every row of X. The table the classifier was
        fitted from (the same object: every row of it, drawn or not) takes the decisions the device returned with the
        fit; any other table is multiplied out on the host from coef_ and intercept_."""
        self._check_fitted()
        if X is self._table:
            return self._table_decisions
        import scipy.sparse
        Xc = X.tocsc() if scipy.sparse.issparse(X) else np.asarray(X)
        if Xc.shape[1] != self.n_features_in_:
            raise ValueError('X has %d features, the classifier was fitted on %d' % (Xc.shape[1], self.n_features_in_))
        return np.array([np.asarray(Xc[:, fs] @ est.coef_[0]).ravel() + est.intercept_[0]
                         for est, fs in zip(self.estimators_, self.estimators_features_)])

    @staticmethod
    def _votes(decisions):
        ones = (decisions > 0).sum(axis=0).astype(np.float64)
        n_est = decisions.shape[0]
        return np.stack([(n_est - ones) / n_est, ones / n_est], axis=1)

    def predict_proba(self, X):
        """(n_samples, 2): the shares of the members voting for classes_[0] / classes_[1] (a member votes classes_[1] where
        its decision is positive) -- what sklearn's BaggingClassifier returns for members without predict_proba."""
        return self._votes(self.decision_function_all(X))

    def predict(self, X):
        """The class with more votes; a tie goes to classes_[0]."""
        proba = self.predict_proba(X)
        return self.classes_[np.argmax(proba, axis=1)]

    def _predict_rows(self, index):
        """(predict, predict_proba) of rows `index` of the table fitted from"""
        proba = self._votes(self._table_decisions[:, index])
        return self.classes_[np.argmax(proba, axis=1)], proba


def _confusion(y_true, y_pred):
    t, p = np.asarray(y_true) != 0, np.asarray(y_pred) != 0
    return int(np.sum(t & p)), int(np.sum(~t & p)), int(np.sum(t & ~p)), int(np.sum(~t & ~p))


def _accuracy(y_true, y_pred):
    tp, fp, fn, tn = _confusion(y_true, y_pred)
    return (tp + tn) / float(tp + fp + fn + tn)


def _precision(y_true, y_pred):
    tp, fp, fn, tn = _confusion(y_true, y_pred)
    return tp / float(tp + fp) if tp + fp else 0.0


def _recall(y_true, y_pred):
    tp, fp, fn, tn = _confusion(y_true, y_pred)
    return tp / float(tp + fn) if tp + fn else 0.0


def _mcc(y_true, y_pred):
    tp, fp, fn, tn = _confusion(y_true, y_pred)
    n = float(tp + fp + fn + tn)
    t_sum = np.array([tn + fp, tp + fn], dtype=np.float64)
    p_sum = np.array([tn + fn, tp + fp], dtype=np.float64)
    cov_ytyp = (tp + tn) * n - np.dot(t_sum, p_sum)
    cov_ypyp = n * n - np.dot(p_sum, p_sum)
    cov_ytyt = n * n - np.dot(t_sum, t_sum)
    if cov_ypyp * cov_ytyt == 0:
        return 0.0
    return cov_ytyp / np.sqrt(cov_ytyt * cov_ypyp)


def _roc_auc(y_true, score):
    """Area under the ROC curve: one point per distinct score descending, interior points collinear with both neighbours
    dropped, rates = counts / totals, trapezoid rule -- the operations of sklearn.metrics.roc_auc_score in its order, so
    the same bits (the mid-rank statistic is the same number only up to the last bit)."""
    t = np.asarray(y_true) != 0
    score = np.asarray(score, dtype=np.float64)
    if t.all() or not t.any():
        raise ValueError('Only one class present in y_true. ROC AUC score is not defined in that case.')
    order = np.argsort(score, kind='stable')[::-1]
    s, t = score[order], t[order]
    idx = np.r_[np.flatnonzero(np.diff(s)), t.size - 1]
    tps = np.cumsum(t.astype(np.float64))[idx]
    fps = 1 + idx - tps
    if fps.size > 2:
        keep = np.flatnonzero(np.r_[True, np.logical_or(np.diff(fps, 2), np.diff(tps, 2)), True])
        fps, tps = fps[keep], tps[keep]
    tps, fps = np.r_[0, tps], np.r_[0, fps]
    fpr, tpr = fps / fps[-1], tps / tps[-1]
    return float((np.diff(fpr) * (tpr[1:] + tpr[:-1]) / 2.0).sum())


def _sir_metrics(y_train, y_train_hat, p_train, y_test, y_test_hat, p_test):
    results = {}
    for metric, name in ((_accuracy, 'Accuracy'), (_precision, 'Precision'), (_recall, 'Recall'), (_mcc, 'MCC')):
        results['Train_' + name] = metric(y_train, y_train_hat)
        results['Test_' + name] = metric(y_test, y_test_hat)
    results['Train_AUC'] = _roc_auc(y_train, p_train[:, 1])
    results['Test_AUC'] = _roc_auc(y_test, p_test[:, 1])
    return results


def __evaluate_sir_model__(clf, X_train, y_train, X_test, y_test):
    """Accuracy, precision, recall, MCC and AUC of a trained binary classifier (labels 0 / 1) on the training and the
    test set, restated in numpy with sklearn's conventions: precision without a positive prediction is 0, MCC with a
    zero denominator is 0, AUC on a single class raises ValueError."""
    return _sir_metrics(y_train, clf.predict(X_train), clf.predict_proba(X_train), y_test, clf.predict(X_test),
                        clf.predict_proba(X_test))


def __extract_weights_from_bagging_ensemble__(clf, feature_labels):
    """The weight of every feature of a bagging ensemble (sklearn's BaggingClassifier of linear models, or a
    BaggedLinearSVC): the mean of its weight over the sub-classifiers that included it; exact zeros are dropped."""
    import pandas as pd
    df_weights_full = {}
    for i, sub_clf in enumerate(clf.estimators_):
        selected_features = clf.estimators_features_[i]
        df_weights_full['CLF' + str(i)] = pd.Series(data=sub_clf.coef_[0], index=selected_features)
    df_weights_full = pd.DataFrame.from_dict(df_weights_full)
    df_weights_full.index = df_weights_full.index.map(lambda x: feature_labels[x])
    df_weights = pd.Series(data=np.nanmean(df_weights_full, axis=1), index=df_weights_full.index)
    return df_weights[df_weights != 0.0]


def _known_amr_ranks(df_weights, case_block_defs, known_amr_drug_set):
    """The rank part of one fold of evaluate_model: block weights expanded to the original features, average and dense
    ranks of |weight| descending, the known AMR features' ranks and the AMR blocks' ranks (printing as the reference)."""
    import pandas as pd
    import scipy.stats
    out = {}
    df_original_weights = {}
    amr_blocks = set()
    for block, weight in df_weights.items():
        block_id = int(block[1:])
        for feature in case_block_defs[block_id]:
            df_original_weights[feature] = weight
            if feature in known_amr_drug_set:
                amr_blocks.add(block)
    df_original_weights = pd.Series(df_original_weights, dtype=np.float64)
    print('\tSelected features:', df_original_weights.shape)
    ranks_avg = scipy.stats.rankdata(-np.abs(df_original_weights.values), method='average')
    ranks_dense = scipy.stats.rankdata(-np.abs(df_original_weights.values), method='dense')
    df_ranks_avg = pd.Series(data=ranks_avg, index=df_original_weights.index, name='ranks_avg')
    df_ranks_dense = pd.Series(data=ranks_dense, index=df_original_weights.index, name='ranks_dense')
    df_ranks = pd.concat([df_ranks_avg, df_ranks_dense], axis=1)
    known_amr_detected = [x for x in df_ranks.index if x in known_amr_drug_set]
    df_ranks_known_amr = df_ranks.reindex(known_amr_detected)
    print('\tSelected known AMR features:', df_ranks_known_amr.shape)
    out['known_AMR_ranks_avg_dense'] = {}
    for feature in df_ranks_known_amr.index:
        out['known_AMR_ranks_avg_dense'][feature] = list(df_ranks_known_amr.loc[feature, :].values)
    block_ranks = scipy.stats.rankdata(-np.abs(df_weights.values), method='average')
    df_block_ranks = pd.Series(data=block_ranks, index=df_weights.index)
    selected_amr_blocks = [x for x in df_weights.index if x in amr_blocks]
    df_block_ranks_amr = df_block_ranks.reindex(selected_amr_blocks)
    print('\tSelected known AMR blocks:', df_block_ranks_amr.shape)
    out['known_AMR_blocks'] = df_block_ranks_amr.to_dict()
    return out


def evaluate_model(base_clf, lsdf_case, case_block_defs, df_amr_org_drug, known_amr_drug_set, n_folds=5, seed=None,
                   folds=None, ctx=None):
    """Prediction performance of a classifier and its recovery of the known AMR genes under stratified cross-validation.

    base_clf           : a BaggedLinearSVC (trained on the device) or any sklearn bagging ensemble of linear models
    lsdf_case          : LightSparseDataFrame, block x genome table (prefilter_features_by_lor / prepare_amr_case_data)
    case_block_defs    : case_block_defs[i] = the features of block i
    df_amr_org_drug    : pd.Series of the genomes' phenotypes (0 / 1), in the table's column order
    known_amr_drug_set : the known AMR features of the drug
    n_folds, seed      : without `folds` the split is sklearn's StratifiedKFold(n_folds, shuffle=True, random_state=seed)
                         (the reference's default seed, a float drawn at import, is refused by current sklearn: None here)
    folds              : list of (train_index, test_index) pairs to use instead; sklearn is then not needed
    ctx                : Context for a BaggedLinearSVC that has none of its own

    Returns {'FOLD1': {...}, ...} with the reference's keys: Train_/Test_ Accuracy, Precision, Recall, MCC, AUC,
    known_AMR_ranks_avg_dense, known_AMR_blocks, Runtime; the reference's lines are printed. With a BaggedLinearSVC all
    folds are fitted by ONE fit_many call, and a fold's Runtime is that call's time divided by the number of folds plus
    the fold's own host work (metrics, weights, ranks). Any other classifier goes fold by fold through
    sklearn.base.clone(base_clf).fit(X_train, y_train), as in the reference.
    """
    X = lsdf_case.data.T.tocsr()
    y = df_amr_org_drug.values.astype(int)
    output = {}
    fold = 1
    if folds is None:
        import sklearn.model_selection
        skf = sklearn.model_selection.StratifiedKFold(n_splits=n_folds, shuffle=True, random_state=seed)
        folds = list(skf.split(X, y))
    device = isinstance(base_clf, BaggedLinearSVC)
    if device:
        clf0 = base_clf if base_clf.ctx is not None or ctx is None else type(base_clf)(**dict(base_clf.get_params(), ctx=ctx))
        t0 = time.time()
        fitted = clf0.fit_many(X, y, [train_index for train_index, _ in folds])
        shared_time = (time.time() - t0) / max(len(folds), 1)
    for i_fold, (train_index, test_index) in enumerate(folds):
        start_time = time.time()
        print('FOLD:', fold)
        fold_id = 'FOLD' + str(fold)
        fold += 1
        output[fold_id] = {}
        print('\tTraining model...')
        y_train, y_test = y[train_index], y[test_index]
        if device:
            clf = fitted[i_fold]
            y_train_hat, p_train = clf._predict_rows(train_index)
            y_test_hat, p_test = clf._predict_rows(test_index)
            prediction_perf = _sir_metrics(y_train, y_train_hat, p_train, y_test, y_test_hat, p_test)
        else:
            import sklearn.base
            X_train, X_test = X[train_index, :], X[test_index, :]
            clf = sklearn.base.clone(base_clf)
            clf.fit(X_train, y_train)
            prediction_perf = __evaluate_sir_model__(clf, X_train, y_train, X_test, y_test)
        for param, value in prediction_perf.items():
            output[fold_id][param] = value
        print('\tAUC (train):', output[fold_id]['Train_AUC'])
        print('\tAUC (test):', output[fold_id]['Test_AUC'])
        df_weights = __extract_weights_from_bagging_ensemble__(clf, lsdf_case.index)
        print('\tSelected blocks:', df_weights.shape)
        output[fold_id].update(_known_amr_ranks(df_weights, case_block_defs, known_amr_drug_set))
        runtime = time.time() - start_time + (shared_time if device else 0.0)
        output[fold_id]['Runtime'] = runtime
        print('\tRuntime:', round(runtime, 3))
    return output


def compute_known_amr_distr(case_block_defs, known_amr_drug_set, selected_blocks=[]):
    """The number of known AMR features and of blocks that hold one, before and (optionally) after LOR filtering.

    case_block_defs    : case_block_defs[i] = the features of block i (prepare_amr_case_data)
    known_amr_drug_set : the known AMR features (prepare_amr_case_data)
    selected_blocks    : the blocks kept, as 'B#' labels (default: none)

    Returns (amr_counts, amr_blocks): amr_counts = (known AMR features, blocks with at least one, known AMR features among
    selected_blocks, selected blocks with at least one); amr_blocks = {block label: its known AMR features}.
    """
    amr_blocks = {}
    for i, block in enumerate(case_block_defs):
        block_amr = [x for x in block if x in known_amr_drug_set]
        if len(block_amr) > 0:
            amr_blocks['B' + str(i)] = block_amr
    n_sel_amr_features = 0
    n_sel_amr_blocks = 0
    for block in selected_blocks:
        if block in amr_blocks:
            n_sel_amr_blocks += 1
            n_sel_amr_features += len(amr_blocks[block])
    return (len(known_amr_drug_set), len(amr_blocks), n_sel_amr_features, n_sel_amr_blocks), amr_blocks
