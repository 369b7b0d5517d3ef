"""TEST MODEL of the bagged linear SVM ensemble (pangenomix_amd/csrc/svm.hip, ml_pipelines.BaggedLinearSVC)
in float64 numpy: the pinned greedy dual coordinate descent, an independent exact solve of the same quadratic programme
(scipy's NNLS on the Cholesky factor), the voting rule of the ensemble and the metrics of evaluate_model. Nothing here
touches a device; sklearn is not imported.

One sub-problem: a binary table X (n genomes x R features), a boolean feature mask, labels y in {0, 1}, multiplicities m
(0 = the genome is not in the training set) and C. Its dual over the genomes with m > 0:
    min 1/2 b'Qb - sum b,  b >= 0,   Q = (y y') * (K + 1) + diag(1 / (2 C m)),   K = Xm Xm'   (Xm = X[:, mask])
"""
import numpy as np


def gram(X, mask):
    Xm = np.asarray(X, dtype=bool)[:, np.asarray(mask, dtype=bool)].astype(np.float64)
    return (Xm @ Xm.T).astype(np.int64)                         # (counts far below 2^53: exact)


def signs(y):
    return np.where(np.asarray(y) != 0, 1.0, -1.0)


def q_matrix(K, y, m, C):
    """(Q over the active genomes, their indices)"""
    m = np.asarray(m)
    act = np.flatnonzero(m > 0)
    s = signs(y)[act]
    Q = np.outer(s, s) * (K[np.ix_(act, act)] + 1.0)
    Q[np.diag_indices_from(Q)] += 1.0 / (2.0 * C * m[act].astype(np.float64))
    return Q, act


def projected(g, b):
    return np.where(b > 0, g, np.minimum(g, 0.0))


def greedy_cd(K, y, m, C, tol=1e-10, max_steps=None):
    """(beta over ALL genomes, steps): the pinned rule. Largest |PG| first (np.argmax: the smallest index among equals),
    d = max(-b_i, -g_i / Q_ii); when the test passes g is recomputed from beta and the test repeated."""
    n = K.shape[0]
    Q, act = q_matrix(K, y, m, C)
    b = np.zeros(act.size)
    g = -np.ones(act.size)
    steps = 0
    if max_steps is None:
        max_steps = 1000000 + 2000 * n
    while True:
        pg = np.abs(projected(g, b))
        i = int(np.argmax(pg))
        if not pg[i] > tol:
            g = Q @ b - 1.0
            pg = np.abs(projected(g, b))
            i = int(np.argmax(pg))
            if not pg[i] > tol:
                break
        if steps >= max_steps:
            raise RuntimeError('more than %d steps' % max_steps)
        d = max(-b[i], -g[i] / Q[i, i])
        b[i] += d
        g += d * Q[:, i]
        steps += 1
    beta = np.zeros(n)
    beta[act] = b
    return beta, steps


def nnls_solve(K, y, m, C):
    """beta over all genomes by an independent method: Q = L L', 1/2 b'Qb - 1'b = 1/2 |L'b - L^-1 1|^2 + const, so the
    optimum is the non-negative least squares solution of L' b = L^-1 1 (Lawson-Hanson active set, exact in exact
    arithmetic)."""
    import scipy.linalg
    import scipy.optimize
    Q, act = q_matrix(K, y, m, C)
    L = np.linalg.cholesky(Q)
    rhs = scipy.linalg.solve_triangular(L, np.ones(act.size), lower=True)
    b, _ = scipy.optimize.nnls(L.T, rhs, maxiter=50 * act.size + 1000)
    beta = np.zeros(K.shape[0])
    beta[act] = b
    return beta


def outputs(X, mask, y, beta):
    """{'coef' [R] (0 outside the mask), 'intercept', 'decision' [n]} of a dual solution"""
    X = np.asarray(X, dtype=bool)
    mask = np.asarray(mask, dtype=bool)
    w = beta * signs(y)
    coef = np.where(mask, X.astype(np.float64).T @ w, 0.0)
    intercept = float(w.sum())
    return {'coef': coef, 'intercept': intercept, 'decision': X[:, mask].astype(np.float64) @ coef[mask] + intercept}


def fit(X, mask, y, m, C, tol=1e-10, max_steps=None, solver='cd'):
    K = gram(X, mask)
    if solver == 'cd':
        beta, steps = greedy_cd(K, y, m, C, tol, max_steps)
    else:
        beta, steps = nnls_solve(K, y, m, C), 0
    out = outputs(X, mask, y, beta)
    out.update(beta=beta, steps=steps)
    return out


def coef_bound(C, m, tol):
    """|beta_i - beta*_i| summed, hence |coef_r - coef*_r| and |intercept - intercept*|, is at most 2 C max(m) n tol for
    the n genomes with m > 0 (strong convexity)."""
    m = np.asarray(m)
    return 2.0 * C * float(m.max()) * int(np.count_nonzero(m)) * tol


def decision_bound(C, m, tol, n_selected):
    return (n_selected + 1) * coef_bound(C, m, tol)


def multiplicities(sample_set, n):
    """bootstrap draws (indices, repeats allowed) -> how often each genome was drawn"""
    return np.bincount(np.asarray(sample_set, dtype=np.int64), minlength=n)


# -- the ensemble's vote (sklearn BaggingClassifier over estimators without predict_proba) ---------------------------------
def vote_proba(decisions):
    """decisions [n_estimators, n_samples] -> [n_samples, 2] vote fractions; an estimator votes 1 where its decision > 0"""
    decisions = np.asarray(decisions)
    ones = (decisions > 0).sum(axis=0).astype(np.float64)
    n_est = decisions.shape[0]
    return np.stack([(n_est - ones) / n_est, ones / n_est], axis=1)


def vote_predict(decisions):
    """argmax of the vote fractions: a tie goes to class 0"""
    return np.argmax(vote_proba(decisions), axis=1)


# -- metrics ------------------------------------------------------------------------------------------------------------
def confusion(y, yhat):
    y, yhat = np.asarray(y) != 0, np.asarray(yhat) != 0
    return (int(np.sum(y & yhat)), int(np.sum(~y & yhat)), int(np.sum(y & ~yhat)), int(np.sum(~y & ~yhat)))    # TP FP FN TN


def accuracy(y, yhat):
    tp, fp, fn, tn = confusion(y, yhat)
    return (tp + tn) / float(tp + fp + fn + tn)


def precision(y, yhat):
    tp, fp, fn, tn = confusion(y, yhat)
    return tp / float(tp + fp) if tp + fp else 0.0


def recall(y, yhat):
    tp, fp, fn, tn = confusion(y, yhat)
    return tp / float(tp + fn) if tp + fn else 0.0


def mcc(y, yhat):
    tp, fp, fn, tn = confusion(y, yhat)
    n = tp + fp + fn + tn
    t = np.array([tn + fp, tp + fn], dtype=np.float64)        # true class sizes
    p = np.array([tn + fn, tp + fp], dtype=np.float64)        # predicted class sizes
    cov_ytyp = float(tp + tn) * n - np.dot(t, p)
    cov_ypyp = float(n) ** 2 - np.dot(p, p)
    cov_ytyt = float(n) ** 2 - np.dot(t, t)
    if cov_ypyp * cov_ytyt == 0:
        return 0.0
    return cov_ytyp / np.sqrt(cov_ytyt * cov_ypyp)


def auc(y, score):
    """Area under the ROC curve as sklearn.metrics.roc_auc_score forms it, bit for bit: one ROC point per distinct score
    (descending), interior points collinear with their neighbours dropped, rates = counts / totals, trapezoid rule. The
    mid-rank statistic (auc_midrank) is the same number up to the last bit only."""
    y = np.asarray(y) != 0
    score = np.asarray(score, dtype=np.float64)
    if y.all() or not y.any():
        raise ValueError('Only one class present in y_true. ROC AUC score is not defined in that case.')
    order = np.argsort(score, kind='stable')[::-1]
    s, t = score[order], y[order]
    idx = np.r_[np.flatnonzero(np.diff(s)), t.size - 1]
    tps = np.cumsum(t.astype(np.float64))[idx]
    fps = 1 + idx - tps
    if fps.size > 2:
        keep = np.flatnonzero(np.r_[True, np.logical_or(np.diff(fps, 2), np.diff(tps, 2)), True])
        fps, tps = fps[keep], tps[keep]
    tps, fps = np.r_[0, tps], np.r_[0, fps]
    fpr, tpr = fps / fps[-1], tps / tps[-1]
    return float((np.diff(fpr) * (tpr[1:] + tpr[:-1]) / 2.0).sum())


def auc_midrank(y, score):
    """(sum of the positives' mid-ranks - n_pos (n_pos + 1) / 2) / (n_pos n_neg)"""
    y = np.asarray(y) != 0
    score = np.asarray(score, dtype=np.float64)
    n_pos, n_neg = int(y.sum()), int((~y).sum())
    order = np.argsort(score, kind='stable')
    s = score[order]
    first = np.flatnonzero(np.r_[True, s[1:] != s[:-1]])
    last = np.r_[first[1:], s.size]
    ranks = np.empty(s.size)
    ranks[order] = np.repeat((first + 1 + last) / 2.0, last - first)
    return (ranks[y].sum() - n_pos * (n_pos + 1) / 2.0) / (float(n_pos) * n_neg)
