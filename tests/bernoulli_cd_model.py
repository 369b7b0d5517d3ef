"""TEST INFRASTRUCTURE: coordinate descent on the Bernoulli grid likelihood (include/pgx.h, "Coordinate descent on that
likelihood"; pangenomix_amd/csrc/bernoulli_cd.hip) restated in numpy, for what runs without a GPU and for
tables of which no fixture exists. Written from the definition in pgx.h, with the device's order of summation and the
same Brent driver, all solves of a sweep side by side in arrays:

    rule around a solve   f at lo and hi; f(lo) f(hi) >= 0: lo when |last - lo| < |last - hi| (strictly), else hi
    brent_many            Brent's method (1973, ch. 4) until half the bracket is below (XTOL + RTOL |b|) / 2 or f(b) == 0,
                          at most MAXITER steps
    row solve             an evaluation adds the absent cells' terms genome after genome (one lane per gene)
    column solve          thread t of COL_THREADS adds the absent genes of the bitmap words t, t + COL_THREADS, ... in
                          ascending order; the partials are folded in halves (d = 128, 64, ..., 1: part[t] += part[t + d])

tests/test_bernoulli_cd_host.py checks it against every fixture of the reference (tests/golden/bernoulli_cd).

TOL = 2 (XTOL + RTOL): two points that each satisfy Brent's stopping rule for the same root (|x| <= 1) lie within
XTOL + RTOL |x| of the sign change each, hence within 4.1e-12 of each other, when the noise of f is negligible
(DESIGN.md 6g has the derivation and the measured difference between this model and the reference)."""
import collections

import numpy as np

XTOL = 2e-12
RTOL = 4 * 2.0 ** -52
MAXITER = 100
COL_THREADS = 256
TOL = 2 * (XTOL + RTOL)

Solves = collections.namedtuple('Solves', 'x evals failed boundary')


def brent_many(f, lo, hi, last):
    """f: array of n points -> array of n values (solve k's function at point k). Returns Solves: the results, the
    evaluations each took (the two at the bounds included), which did not converge, which took the boundary rule."""
    n = last.size
    a, b = np.full(n, lo, dtype=np.float64), np.full(n, hi, dtype=np.float64)
    fa, fb = f(a), f(b)
    evals = np.full(n, 2, dtype=np.int64)
    boundary = fa * fb >= 0.0
    x = np.where(np.abs(last - lo) < np.abs(last - hi), lo, hi).astype(np.float64)
    active = ~boundary
    failed = np.zeros(n, dtype=bool)
    steps = np.zeros(n, dtype=np.int64)
    c, fc = a.copy(), fa.copy()
    d = b - a
    e = d.copy()
    with np.errstate(all='ignore'):
        while active.any():
            same = ((fb > 0.0) & (fc > 0.0)) | ((fb < 0.0) & (fc < 0.0))
            c, fc = np.where(same, a, c), np.where(same, fa, fc)
            d, e = np.where(same, b - a, d), np.where(same, b - a, e)
            swap = np.abs(fc) < np.abs(fb)
            a, b, c = np.where(swap, b, a), np.where(swap, c, b), np.where(swap, b, c)
            fa, fb, fc = np.where(swap, fb, fa), np.where(swap, fc, fb), np.where(swap, fb, fc)
            tol1 = (XTOL + RTOL * np.abs(b)) / 2.0
            xm = (c - b) / 2.0
            stop = active & ((np.abs(xm) < tol1) | (fb == 0.0))
            x[stop] = b[stop]
            active = active & ~stop
            late = active & (steps == MAXITER)
            x[late] = b[late]
            failed |= late
            active = active & ~late
            if not active.any():
                break
            steps += active
            interpolate = (np.abs(e) >= tol1) & (np.abs(fa) > np.abs(fb))
            s = fb / fa
            qq, r = fa / fc, fb / fc
            secant = a == c
            p = np.where(secant, 2.0 * xm * s, s * (2.0 * xm * qq * (qq - r) - (b - a) * (r - 1.0)))
            q = np.where(secant, 1.0 - s, (qq - 1.0) * (r - 1.0) * (s - 1.0))
            q = np.where(p > 0.0, -q, q)
            p = np.abs(p)
            accept = interpolate & (2.0 * p < np.minimum(3.0 * xm * q - np.abs(tol1 * q), np.abs(e * q)))
            d_new = np.where(accept, p / q, xm)
            e = np.where(accept, d, d_new)
            d = d_new
            a, fa = b.copy(), fb.copy()
            b = np.where(active, b + np.where(np.abs(d) > tol1, d, np.where(xm > 0.0, tol1, -tol1)), b)
            fb = np.where(active, f(b), fb)
            evals += active
    return Solves(x, evals, failed, boundary)


def _row_function(absent, cnt, other, ex_other, use_logs):
    """f of every gene's solve at once: the absent cells' terms added genome after genome"""
    def f(x):
        acc = np.zeros(x.size)
        for j in range(absent.shape[1]):
            if use_logs:
                term = ex_other[j] / (-np.expm1(x + other[j]))
            else:
                term = other[j] / (1.0 - x * other[j])
            acc = np.where(absent[:, j], acc + term, acc)
        return cnt * np.exp(-x) - acc if use_logs else cnt / x - acc
    return f


def _col_function(absent, cnt, other, ex_other, use_logs):
    """f of every genome's solve at once: per-thread partials over the thread's words, folded in halves"""
    G, S = absent.shape
    words = -(-G // 64)

    def f(x):
        part = np.zeros((COL_THREADS, S))
        for w0 in range(0, words, COL_THREADS):
            for bit in range(64):
                genes = (w0 + np.arange(COL_THREADS)) * 64 + bit
                t = np.nonzero(genes < G)[0]
                if t.size == 0:
                    continue
                i = genes[t]
                if use_logs:
                    term = ex_other[i][:, None] / (-np.expm1(x[None, :] + other[i][:, None]))
                else:
                    term = other[i][:, None] / (1.0 - x[None, :] * other[i][:, None])
                part[t] = np.where(absent[i], part[t] + term, part[t])
        d = COL_THREADS // 2
        while d:
            part[:d] += part[d:2 * d]
            d //= 2
        return cnt * np.exp(-x) - part[0] if use_logs else cnt / x - part[0]
    return f


def sweep_rows(X, pq, lo, hi, use_logs):
    """One row sweep: Solves for the genes from the solver's variables pq = [P; Q] (or their logs; lo, hi likewise)."""
    X = np.asarray(X, dtype=bool)
    G = X.shape[0]
    with np.errstate(all='ignore'):
        f = _row_function(~X, X.sum(1).astype(np.float64), pq[G:], np.exp(pq[G:]), use_logs)
        return brent_many(f, lo, hi, pq[:G])


def sweep_cols(X, pq, lo, hi, use_logs):
    X = np.asarray(X, dtype=bool)
    G = X.shape[0]
    with np.errstate(all='ignore'):
        f = _col_function(~X, X.sum(0).astype(np.float64), pq[:G], np.exp(pq[:G]), use_logs)
        return brent_many(f, lo, hi, pq[G:])


def likelihood(X, pq, use_logs):
    """The per-cell likelihood at the solver's variables, (LL, sum of the absolute terms, present cells): float64 p q and
    1 - p q (lp + lq in the log flavour), the logs and the sum in longdouble."""
    X = np.asarray(X, dtype=bool)
    G = X.shape[0]
    L = np.longdouble
    if use_logs:
        s = pq[:G, None] + pq[None, G:]
        terms = np.where(X, s.astype(L), np.log(-np.expm1(s.astype(L))))
    else:
        r = pq[:G, None] * pq[None, G:]
        t = 1.0 - r
        terms = np.where(X, np.log(r.astype(L)), np.log(t.astype(L)))
    return float(terms.sum()), float(np.abs(terms).sum()), int(X.sum())


def ll_bound(scale, present):
    """DESIGN.md 6a's accuracy rule"""
    return 1e-12 * scale + 2.0 ** -52 * present


def ll_gradient(X, pq, use_logs):
    """dLL / d(solver variable) of every coordinate, by numpy at the point pq"""
    X = np.asarray(X, dtype=bool)
    G = X.shape[0]
    if use_logs:
        s = pq[:G, None] + pq[None, G:]
        per_cell = np.where(X, 1.0, np.exp(s) / np.expm1(s))          # d/ds of s and of log(-expm1(s))
        return np.concatenate((per_cell.sum(1), per_cell.sum(0)))
    r = pq[:G, None] * pq[None, G:]
    t = 1.0 - r
    gp = X.sum(1) / pq[:G] - np.where(X, 0.0, pq[None, G:] / t).sum(1)
    gq = X.sum(0) / pq[G:] - np.where(X, 0.0, pq[:G, None] / t).sum(0)
    return np.concatenate((gp, gq))


Run = collections.namedtuple('Run', 'table solver evals failed boundary')


def run(X, init_p, init_q, lo, hi, n_iterations, use_logs=False):
    """pgx_bernoulli_cd on a dense bool table: table and solver table [1 + G + S, n_iterations + 1]; the evaluations,
    failures and boundary flags of every solve, [n_iterations, G + S]."""
    X = np.asarray(X, dtype=bool)
    G, S = X.shape
    n = G + S
    pq = np.concatenate((np.asarray(init_p, dtype=np.float64), np.full(S, float(init_q))))
    if use_logs:
        pq, lo, hi = np.log(pq), np.log(lo), np.log(hi)
    table, solver = np.zeros((1 + n, n_iterations + 1)), np.zeros((1 + n, n_iterations + 1))
    evals, failed = np.zeros((n_iterations, n), dtype=np.int64), np.zeros((n_iterations, n), dtype=bool)
    boundary = np.zeros((n_iterations, n), dtype=bool)
    for it in range(n_iterations + 1):
        if it:
            rows = sweep_rows(X, pq, lo, hi, use_logs)
            pq = np.concatenate((rows.x, pq[G:]))
            cols = sweep_cols(X, pq, lo, hi, use_logs)
            pq = np.concatenate((pq[:G], cols.x))
            evals[it - 1] = np.concatenate((rows.evals, cols.evals))
            failed[it - 1] = np.concatenate((rows.failed, cols.failed))
            boundary[it - 1] = np.concatenate((rows.boundary, cols.boundary))
        ll = likelihood(X, pq, use_logs)[0]
        solver[0, it], solver[1:, it] = ll, pq
        table[0, it], table[1:, it] = ll, np.exp(pq) if use_logs else pq
    return Run(table, solver, evals, failed, boundary)


def dense(rows, cols, shape):
    X = np.zeros(tuple(int(v) for v in shape), dtype=bool)
    X[np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)] = True
    return X
