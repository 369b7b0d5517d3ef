"""TEST INFRASTRUCTURE: the Bernoulli grid likelihood (include/pgx.h, "Bernoulli grid likelihood";
pangenomix_amd/csrc/bernoulli.hip) restated without a GPU, for tables of which no fixture of the reference
exists. tests/test_bernoulli_host.py checks it against every fixture and against exact(), so it is a fair yardstick.

    geometry(G, S)      make_geom() of bernoulli.hip restated: the slab split of passes A and B and the workspace size
    evaluate(table, pq) the model as pgx.h defines it: r = fl(p q) and t = fl(1 - r) in float64 (that rounding is part of
                        the contract), every log, quotient and sum in np.longdouble, cell by cell with
                            present:  log r + 0 * log t          0 / t          0 / t
                            absent:   0 * log r + log t          q / t          p / t
                        so that nan and inf come out where the per-cell expressions put them. Row blocks of BLOCK_CELLS
                        cells: a 70,001 x 400 table never holds more than a few tens of MB.
    exact(X, pq)        LL and gradient with 50 digits (mpmath) and the TRUE product p q, for tables of a few thousand
                        cells whose products all lie inside (0, 1)

Tolerances (u = 2^-53; DESIGN.md 6a "Accuracy"):
    ll_bound_reference  |LL - sum log(fl(p q)) ...| <= 1e-12 x ll_scale + 2 u x (present cells): fl(p q) carries a
                        relative error of u, which log turns into an absolute one of u per present cell, whatever the size
                        of log(p q) -- and |log(p q)| is about 1e-8 near the upper bound. The fast mode's
                        rowsum log p + colsum log q does not carry it, the reference's log(fl(p q)) does.
    ll_bound_exact      evaluate() against exact(): an absent cell's log(1 - fl(p q)) moves by u r / t for the same
                        reason, hence 1e-12 x ll_scale + 2 u x (present cells + sum over absent cells of r / t). This
                        holds where fl(1 - r) is exact (r >= 1/2, Sterbenz; every point inside prob_bounds >= 0.8); below
                        that 1 - r rounds by up to u / 2 absolute, which r / t < 1 does not cover.
"""
import collections

import numpy as np

U = 2.0 ** -53
BLOCK_CELLS = 1 << 18                                        # x 16 bytes x about ten temporaries
LD = np.longdouble

# bernoulli.hip: BN_THREADS, BN_TARGET_WAVES, BN_MIN_SPAN
THREADS, TARGET_WAVES, MIN_SPAN = 256, 4096, 16

# G x S of tests/test_gpu_bernoulli_geometry.py: the smallest tables that reach each class of
# test_bernoulli_host.test_geometry_shapes_cover_every_class
GEOMETRY_SHAPES = [(300, 17), (300, 40), (257, 257), (64, 1100), (16001, 1025), (52545, 257), (70001, 400)]

Geometry = collections.namedtuple(
    'Geometry', 'words a_slabs a_span a_last a_by_waves a_blocks b_slabs b_span b_last b_blocks workspace_bytes')


def _ceil_div(a, b):
    return -(-a // b)


def _align256(x):
    return (x + 255) & ~255


def geometry(G, S):
    """a_last / b_last: genomes / words in the last slab of pass A / B; a_by_waves: the wave target, not S / MIN_SPAN,
    limits a_slabs; a_blocks / b_blocks: workgroups in x."""
    words = _ceil_div(G, 64)
    by_waves, by_span = _ceil_div(TARGET_WAVES, _ceil_div(G or 1, 64)), max(1, _ceil_div(S, MIN_SPAN))
    a_span = max(1, _ceil_div(S, min(by_waves, by_span)))
    a_slabs = max(1, _ceil_div(S, a_span))
    slabs = min(_ceil_div(TARGET_WAVES, _ceil_div(S or 1, 64)), max(1, words))
    b_span = max(1, _ceil_div(words, slabs))
    b_slabs = max(1, _ceil_div(words, b_span))
    o = 256                                                  # the mode word
    for n in (a_slabs * G * 8, a_slabs * G * 8, a_slabs * G * 4, b_slabs * S * 8, b_slabs * S * 4, (G + S) * 8):
        o = _align256(o + n)
    return Geometry(words, a_slabs, a_span, S - (a_slabs - 1) * a_span, by_waves < by_span, _ceil_div(G, THREADS),
                    b_slabs, b_span, words - (b_slabs - 1) * b_span, _ceil_div(S, THREADS), o)


Evaluation = collections.namedtuple('Evaluation', 'll grad scale ll_scale present absent_rt')


def _row_blocks(table):
    """(first row, bool block) of a dense 2-D table or of COO coordinates (rows, cols, (G, S))."""
    if isinstance(table, tuple):
        rows, cols, (G, S) = table
        rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
        if np.any(rows[1:] < rows[:-1]):
            order = np.argsort(rows, kind='stable')
            rows, cols = rows[order], cols[order]
        step = max(1, BLOCK_CELLS // max(S, 1))
        for i0 in range(0, G, step):
            i1 = min(G, i0 + step)
            a, b = np.searchsorted(rows, (i0, i1))
            X = np.zeros((i1 - i0, S), dtype=bool)
            X[rows[a:b] - i0, cols[a:b]] = True
            yield i0, X
    else:
        X = np.asarray(table) != 0
        step = max(1, BLOCK_CELLS // max(X.shape[1], 1))
        for i0 in range(0, X.shape[0], step):
            yield i0, X[i0:i0 + step]


def shape_of(table):
    return tuple(int(v) for v in (table[2] if isinstance(table, tuple) else np.asarray(table).shape))


def _zero_times_log(x):
    """0 * log(x) of a float64 x: 0 for a finite x > 0; nan for 0 (0 * -inf), inf (0 * inf), a negative x and nan."""
    return np.where((x > 0) & (x < np.inf), 0.0, np.nan)


def _zero_over(t):
    """0 / t: a zero (its sign changes no sum) unless t is 0 or nan."""
    return np.where((t != 0) & ~np.isnan(t), 0.0, np.nan)


def _evaluate_block(X, P, Q):
    """One row block. The logs and quotients (longdouble) are taken only in the cells whose term they are; the other
    half of each per-cell expression is the 0 * log or 0 / t above, which float64 tells exactly (summed on its own: a
    sum of zeros and nans)."""
    A = ~X
    r = P[:, None] * Q[None, :]                              # float64: one rounding each
    t = 1.0 - r
    shape = X.shape
    own = np.zeros(shape, LD)                                # log r where present, log t where absent
    np.log(r, out=own, where=X, dtype=LD)
    np.log(t, out=own, where=A, dtype=LD)
    ll = own.sum() + LD(np.where(X, _zero_times_log(t), _zero_times_log(r)).sum())
    ll_scale = np.abs(own, out=own).sum()
    zt = np.where(X, _zero_over(t), 0.0)
    sums = []
    for num in (Q.astype(LD)[None, :], P.astype(LD)[:, None], r):
        quot = np.zeros(shape, LD)                           # q / t, p / t, r / t where absent
        np.divide(np.broadcast_to(num, shape), t, out=quot, where=A, dtype=LD)
        sums.append(quot)
    gp, gq, rt = sums
    dp, dq = gp.sum(1) + zt.sum(1), gq.sum(0) + zt.sum(0)
    return (ll, ll_scale, rt.sum(), dp, dq, np.abs(gp, out=gp).sum(1), np.abs(gq, out=gq).sum(0), X.sum(1), X.sum(0))


def evaluate(table, pq, threads=16):
    """Evaluation(ll, grad [G + S], scale [G + S], ll_scale, present, absent_rt), float64 each: scale and ll_scale are the
    sums of the absolute values of each gradient entry's and of LL's terms (point_scale and point_ll_scale of the
    fixtures), present the number of present cells, absent_rt the sum of r / t over the absent ones. Row blocks run on
    `threads` threads; their results are added in row order, whatever the number of threads."""
    import concurrent.futures
    G, S = shape_of(table)
    pq = np.asarray(pq, dtype=np.float64)
    assert pq.shape == (G + S,)
    P, Q = pq[:G], pq[G:]
    ll = ll_scale = absent_rt = LD(0)
    dp, sp, rowsum = np.zeros(G, LD), np.zeros(G, LD), np.zeros(G, np.int64)
    dq, sq, colsum = np.zeros(S, LD), np.zeros(S, LD), np.zeros(S, np.int64)

    def job(block):
        with np.errstate(all='ignore'):
            return block[0], _evaluate_block(block[1], P[block[0]:block[0] + block[1].shape[0]], Q)

    with concurrent.futures.ThreadPoolExecutor(max_workers=threads) as pool, np.errstate(all='ignore'):
        for i0, (b_ll, b_scale, b_rt, b_dp, b_dq, b_sp, b_sq, b_rows, b_cols) in pool.map(job, _row_blocks(table)):
            i1 = i0 + b_rows.size
            ll, ll_scale, absent_rt = ll + b_ll, ll_scale + b_scale, absent_rt + b_rt
            dp[i0:i1], sp[i0:i1], rowsum[i0:i1] = b_dp, b_sp, b_rows
            dq, sq, colsum = dq + b_dq, sq + b_sq, colsum + b_cols
        lead = np.concatenate((rowsum, colsum)).astype(LD) / pq.astype(LD)
        grad = lead - np.concatenate((dp, dq))
        scale = np.abs(lead) + np.concatenate((sp, sq))
        return Evaluation(np.float64(ll), grad.astype(np.float64), scale.astype(np.float64), np.float64(ll_scale),
                          int(rowsum.sum()), np.float64(absent_rt))


def exact(X, pq):
    """(LL, gradient) rounded from 50 digits, with the true p q."""
    import mpmath
    X = np.asarray(X) != 0
    G, S = X.shape
    assert G * S <= 10000 and len(pq) == G + S
    with mpmath.workdps(50):
        P, Q = [mpmath.mpf(float(v)) for v in pq[:G]], [mpmath.mpf(float(v)) for v in pq[G:]]
        ll, dp, dq = mpmath.mpf(0), [mpmath.mpf(0)] * G, [mpmath.mpf(0)] * S
        for i in range(G):
            for j in range(S):
                r = P[i] * Q[j]
                if not 0 < r < 1:
                    raise ValueError('exact() takes products inside (0, 1)')
                if X[i, j]:
                    ll += mpmath.log(r)
                    dp[i] += 1 / P[i]
                    dq[j] += 1 / Q[j]
                else:
                    ll += mpmath.log(1 - r)
                    dp[i] -= Q[j] / (1 - r)
                    dq[j] -= P[i] / (1 - r)
        return float(ll), np.array([float(v) for v in dp + dq])


def ll_bound_reference(ev):
    return 1e-12 * ev.ll_scale + 2 * U * ev.present


def ll_bound_exact(ev):
    return 1e-12 * ev.ll_scale + 2 * U * (ev.present + ev.absent_rt)


def same_specials(got, want):
    got, want = np.atleast_1d(got), np.atleast_1d(want)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_array_equal(np.isposinf(got), np.isposinf(want))
    np.testing.assert_array_equal(np.isneginf(got), np.isneginf(want))


def assert_evaluation(out, ev, label=''):
    """out = [LL; gradient] of the device against evaluate(): specials in the same places, LL within
    ll_bound_reference, every finite gradient entry within 1e-12 x its scale. Returns (LL error, LL bound)."""
    same_specials(out[:1], ev.ll)
    same_specials(out[1:], ev.grad)
    err_ll = bound = 0.0
    if np.isfinite(ev.ll):
        err_ll, bound = abs(float(out[0]) - float(ev.ll)), ll_bound_reference(ev)
        assert err_ll <= bound, (label, err_ll, bound)
    fin = np.isfinite(ev.grad)
    err = np.abs(out[1:][fin] - ev.grad[fin])
    assert np.all(err <= 1e-12 * ev.scale[fin]), (label, float((err / ev.scale[fin]).max()))
    return err_ll, bound


# ---- the tables and points of the value-edge tests (tests/test_gpu_bernoulli_edges.py, tests/test_bernoulli_host.py) -----
EDGE_SHAPES = [(65, 7), (128, 12)]
BOUNDS = (0.8, 0.99999999)                                   # compute_bernoulli_grid_core_genome's default prob_bounds


def random_table(rng, G, S, absent=0.1):
    """About `absent` of the cells absent, one all-ones row and one all-zero row (bool [G, S])."""
    X = rng.random((G, S)) >= absent
    if G >= 3:
        X[G // 3], X[(2 * G) // 3] = True, False
    return X


def edge_tables(G, S):
    rng = np.random.default_rng(1000 * G + S)
    one_zero = np.ones((G, S), dtype=bool)
    one_zero[G - 1, S // 2] = False                          # (the last gene: the last valid bit of the last word)
    column = rng.random((G, S)) < 0.5
    column[:, S - 2] = True
    return {'all_ones': np.ones((G, S), dtype=bool), 'all_zeros': np.zeros((G, S), dtype=bool), 'one_zero': one_zero,
            'ones_column': column}


def edge_points(X):
    """The start point of compute_bernoulli_grid_core_genome's default call, everything on the upper and on the lower
    bound, and P, Q in [0.9999999, 0.99999999]."""
    G, S = X.shape
    lo, hi = BOUNDS
    rng = np.random.default_rng(7 * G + S)
    start = np.clip(np.concatenate((X.sum(1) / float(S), 0.9999 * np.ones(S))), lo, hi)
    return {'start': start, 'upper': np.full(G + S, hi), 'lower': np.full(G + S, lo),
            'near_one': rng.uniform(0.9999999, 0.99999999, G + S)}


def interior_and_bounds_points(rng, n):
    lo, hi = BOUNDS
    edges = rng.uniform(lo, hi, n)
    edges[::3], edges[1::3] = lo, hi
    return {'interior': rng.uniform(lo, lo + 0.999 * (hi - lo), n), 'bounds': edges}
