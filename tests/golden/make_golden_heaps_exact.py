"""Writes tests/golden/next/exact_heaps.npz: pan tables (int32) with the EXACT least-squares Heaps fit of every row.

Own code, no reference involved: the minimiser of  sum_j (kappa j^alpha - y_j)^2,  j = 1..S,  is computed with mpmath at
60 digits and rounded to float64 -- kappa is eliminated in closed form (kappa(alpha) = sum y x^alpha / sum x^(2 alpha)),
the stationarity equation in alpha,  sum_j (kappa(alpha) x_j^alpha - y_j) x_j^alpha log x_j = 0,  is solved by findroot
and checked to be a minimum (its derivative is positive there).

Per row the file also holds the FLOOR: how far a float64 numpy restatement of libpgx's fit (csrc/heaps.hip: start
(0.5, min of the row), 2 x 2 normal equations, damping x 10 / x 0.1, the same two stopping rules and the 200-step cap,
then the undamped Gauss-Newton polish), run here on the CPU in four rounding variants (VARIANTS), ends from that
minimiser at most -- relative in alpha and kappa (absolute in alpha where the exact alpha is 0). The floor is measured on this restatement, never on the device. The tolerance the tests
use is  rtol = MARGIN x the largest floor  (MARGIN = 64: the device's pow and log may differ from libm's by a few ulp
and its wave sums run in another order, and the problem's conditioning multiplies that); it is stored as `rtol` and
must not exceed RTOL_CAP = 1e-9. A row whose floor forces more is ill-conditioned and has to be replaced: the script
refuses to write the file then.

Rows (table name -> what it covers):
  noisy_s<S>        three noisy monotone power-law curves each at S = 2, 3, 63, 64, 65, 127, 128, 130, 400, 513
                    (the kernel's lanes stride by 64: the tails j >= 64 floor(S / 64), one to three rounds per lane)
  misfit_s<S>       at S = 65, 130, 400: two power laws with an offset, a logarithm, a power law with 3 % scatter -- real
                    residuals, which make the point of convergence depend on the Jacobian
  exact_rounded     1234.5 j^0.37 rounded to integers
  flat              a constant curve: alpha = 0 exactly (compared absolutely), kappa = the constant
  near_int32_max    counts up to 2^31 - 1
  alpha_above_one   a super-linear curve (alpha = 1.3)
  far_start         one point of the curve is 3, so the start (0.5, 3) is four orders of magnitude from kappa
An all-zero row has no unique minimiser and stays with the fixtures of make_golden_next.py.

  python tests/golden/make_golden_heaps_exact.py           writes the file
  python tests/golden/make_golden_heaps_exact.py --check   recomputes everything and compares with the committed file
"""
import os
import sys

import mpmath
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, 'next', 'exact_heaps.npz')      # (not heaps_*.npz: those are the reference-made fixtures the older tests glob)
MARGIN = 64.0
RTOL_CAP = 1e-9
INT32_MAX = 2 ** 31 - 1
NOISE = 2e-4        # relative scatter of the noisy curves (rounding to integers adds about as much at these sizes)


def _wave_sum(v):
    """the kernel's order: lane l adds its elements l, l + 64, ... one after the other, then a butterfly over the lanes"""
    acc = np.zeros(64)
    for j0 in range(0, v.size, 64):
        chunk = v[j0:j0 + 64]
        acc[:chunk.size] += chunk
    d = 32
    while d:
        acc = acc + acc[np.arange(64) ^ d]
        d >>= 1
    return float(acc[0])


# Rounding variants of the restatement: the floor is the farthest any of them ends from the minimiser, so that it does
# not hang on how one order of summation or one pow happens to round.
VARIANTS = (
    (lambda v: float(np.sum(v)), np.power),                                    # numpy's pairwise sum, libm's pow
    (lambda v: float(np.sum(v[::-1])), np.power),                              # the other way round
    (lambda v: float(np.sum(v)), lambda x, a: np.exp(a * np.log(x))),          # pow as exp(a log x)
    (_wave_sum, np.power),                                                     # the kernel's order of summation
)


def lm_restatement(y, variant=0):
    """csrc/heaps.hip's fit in float64 numpy -- the damped loop, then the undamped Gauss-Newton polish: (alpha, kappa,
    outer steps of the damped loop)."""
    total, power = VARIANTS[variant]
    y = np.asarray(y, dtype=np.float64)
    x = np.arange(1, y.size + 1, dtype=np.float64)
    lx = np.log(x)

    def cost_of(aa, kk):
        r = kk * power(x, aa) - y
        return total(r * r)

    def normal_equations(a, k):
        p = power(x, a)
        r = k * p - y
        da, dk = k * p * lx, p
        return total(da * da), total(da * dk), total(dk * dk), total(da * r), total(dk * r)

    with np.errstate(over='ignore', invalid='ignore'):   # (a step that overshoots costs inf and is refused, as on the device)
        a, k = 0.5, float(y.min())
        cost, lam = cost_of(a, k), 1e-3
        n = 0
        while n < 200:
            saa, sak, skk, ga, gk = normal_equations(a, k)
            done = False
            for tries in range(40):
                m00, m11 = saa * (1.0 + lam), skk * (1.0 + lam)
                det = m00 * m11 - sak * sak
                if not abs(det) > 0.0:
                    lam *= 10.0
                    continue
                d_a, d_k = -(m11 * ga - sak * gk) / det, -(m00 * gk - sak * ga) / det
                c2 = cost_of(a + d_a, k + d_k)
                if c2 <= cost:
                    small = abs(d_a) <= 1e-14 * (abs(a) + 1e-14) and abs(d_k) <= 1e-14 * (abs(k) + 1e-14)
                    flat = cost - c2 <= 1e-16 * cost
                    a, k, cost = a + d_a, k + d_k, c2
                    lam = max(lam * 0.1, 1e-12)
                    done = small or flat
                    break
                lam *= 10.0
                if tries == 39:
                    done = True
            if done:
                break
            n += 1
        prev = np.inf
        for _ in range(30):
            saa, sak, skk, ga, gk = normal_equations(a, k)
            det = saa * skk - sak * sak
            if not abs(det) > 0.0:
                break
            d_a, d_k = -(skk * ga - sak * gk) / det, -(saa * gk - sak * ga) / det
            size = max(abs(d_a) / (abs(a) + 1e-14), abs(d_k) / (abs(k) + 1e-14))
            if not size <= 1e-6 or size >= prev:
                break
            a, k, prev = a + d_a, k + d_k, size
            if size <= 1e-15:
                break
    return a, k, n


def exact_minimiser(y, a_start):
    """(alpha, kappa) as mpmath numbers: the root of the reduced stationarity equation next to a_start."""
    mpmath.mp.dps = 60
    ys = [mpmath.mpf(int(v)) for v in y]
    lx = [mpmath.log(j + 1) for j in range(len(ys))]

    def kappa_of(a):
        p = [mpmath.exp(a * l) for l in lx]
        return mpmath.fsum(v * q for v, q in zip(ys, p)) / mpmath.fsum(q * q for q in p)

    def g(a):
        p = [mpmath.exp(a * l) for l in lx]
        k = mpmath.fsum(v * q for v, q in zip(ys, p)) / mpmath.fsum(q * q for q in p)
        return mpmath.fsum((k * q - v) * q * l for v, q, l in zip(ys, p, lx))

    a = mpmath.findroot(g, mpmath.mpf(a_start), tol=mpmath.mpf(10) ** -45, maxsteps=200)
    if abs(a) < mpmath.mpf(10) ** -30:          # (the flat row: the root is 0 itself)
        a = mpmath.mpf(0)
    assert mpmath.diff(g, a) > 0, 'not a minimum'
    return a, kappa_of(a)


def fit_and_floor(y):
    """(alpha, kappa) exact as float64, the restatement's largest relative distance from them over its rounding variants
    (alpha, kappa), the damped loop's largest step count"""
    fits = [lm_restatement(y, v) for v in range(len(VARIANTS))]
    a, k = exact_minimiser(y, fits[0][0])
    fa = max(float(abs(mpmath.mpf(f[0]) - a) / (abs(a) if a != 0 else 1)) for f in fits)
    fk = max(float(abs(mpmath.mpf(f[1]) - k) / abs(k)) for f in fits)
    return float(a), float(k), fa, fk, max(f[2] for f in fits)


def monotone_int(v):
    return np.maximum.accumulate(np.clip(np.rint(v), 1, INT32_MAX)).astype(np.int64)


def tables():
    """name -> int64 [rows, S] (values within int32)"""
    out = {}
    for S in (2, 3, 63, 64, 65, 127, 128, 130, 400, 513):
        rng = np.random.default_rng(1000 + S)
        x = np.arange(1, S + 1, dtype=np.float64)
        rows = []
        while len(rows) < 3:
            kappa, alpha = rng.uniform(500.0, 5000.0), rng.uniform(0.2, 0.7)
            y = monotone_int(kappa * x ** alpha * (1.0 + NOISE * rng.standard_normal(S)))
            if S == 2:                            # (two equal points would be a flat row: keep these strictly rising)
                y = y + np.array([0, 1])
            # a draw whose floor would push MARGIN x floor over RTOL_CAP is ill-conditioned and the next draw takes its
            # place (none is, since the fit ends with its Gauss-Newton polish)
            f = fit_and_floor(y)
            if MARGIN * max(f[2], f[3]) > RTOL_CAP:
                print('noisy_s%d: a draw with floor %.2e is replaced' % (S, max(f[2], f[3])))
                continue
            rows.append(y)
        out['noisy_s%d' % S] = np.array(rows)
    # curves a power law does NOT fit: residuals of per cents, largest at the first genomes. A Jacobian that is slightly
    # wrong moves the point such a fit converges to (by its error times the relative residual), where it leaves the fit
    # of a curve without residual alone
    rng = np.random.default_rng(42)
    for S in (65, 130, 400):
        x = np.arange(1, S + 1, dtype=np.float64)
        rows = []
        for offset in (0.3, 1.0):                 # kappa j^alpha + offset x kappa
            kappa, alpha = rng.uniform(500.0, 5000.0), rng.uniform(0.3, 0.7)
            rows.append(monotone_int(kappa * x ** alpha + offset * kappa))
        rows.append(monotone_int(rng.uniform(500.0, 5000.0) * 3.0 * np.log1p(x)))              # a logarithm
        kappa, alpha = rng.uniform(500.0, 5000.0), rng.uniform(0.3, 0.7)
        rows.append(monotone_int(kappa * x ** alpha * (1.0 + 0.03 * rng.standard_normal(S))))  # 3 % scatter
        out['misfit_s%d' % S] = np.array(rows)
    x = np.arange(1, 201, dtype=np.float64)
    out['exact_rounded'] = np.rint(1234.5 * x ** 0.37).astype(np.int64)[None, :]
    out['flat'] = np.full((1, 100), 777, dtype=np.int64)
    rng = np.random.default_rng(7)
    x = np.arange(1, 301, dtype=np.float64)
    top = INT32_MAX / 300.0 ** 0.25
    near = monotone_int(top * x ** 0.25 * (1.0 + NOISE * rng.standard_normal(300)))
    near[-1] = INT32_MAX
    out['near_int32_max'] = near[None, :]
    x = np.arange(1, 151, dtype=np.float64)
    out['alpha_above_one'] = monotone_int(300.0 * x ** 1.3 * (1.0 + NOISE * rng.standard_normal(150)))[None, :]
    x = np.arange(1, 121, dtype=np.float64)
    far = monotone_int(40000.0 * x ** 0.9 * (1.0 + NOISE * rng.standard_normal(120)))
    far[7] = 3
    out['far_start'] = far[None, :]
    return out


def compute():
    names, arrays, worst = [], {}, 0.0
    for name, tab in tables().items():
        assert tab.min() >= 0 and tab.max() <= INT32_MAX
        alpha, kappa, f_alpha, f_kappa, steps = [], [], [], [], []
        for y in tab:
            a, k, fa, fk, n = fit_and_floor(y)
            assert n < 200, '%s: the restated loop hit its cap' % name
            alpha.append(a), kappa.append(k), f_alpha.append(fa), f_kappa.append(fk), steps.append(n)
            print('%-16s S=%-4d alpha=%.17g kappa=%.17g floor=(%.2e, %.2e) steps=%d' % (name, y.size, a, k, fa, fk, n))
        names.append(name)
        arrays['pan_' + name] = tab.astype(np.int32)
        arrays['alpha_' + name] = np.array(alpha)
        arrays['kappa_' + name] = np.array(kappa)
        arrays['floor_alpha_' + name] = np.array(f_alpha)
        arrays['floor_kappa_' + name] = np.array(f_kappa)
        arrays['steps_' + name] = np.array(steps, dtype=np.int32)
        if MARGIN * max(f_alpha + f_kappa) > RTOL_CAP:
            raise SystemExit('%s: floor %.3g x %g exceeds %g -- ill-conditioned row, replace it'
                             % (name, max(f_alpha + f_kappa), MARGIN, RTOL_CAP))
        worst = max([worst] + f_alpha + f_kappa)
    arrays['names'] = np.array(names)
    arrays['margin'] = np.float64(MARGIN)
    arrays['rtol'] = np.float64(MARGIN * worst)
    print('largest floor %.3e -> rtol %.3e' % (worst, MARGIN * worst))
    return arrays


def main(argv):
    arrays = compute()
    if '--check' in argv:
        z = np.load(OUT)
        assert sorted(z.files) == sorted(arrays), 'the committed file holds other arrays'
        for k, v in arrays.items():
            assert z[k].dtype == np.asarray(v).dtype and np.array_equal(z[k], v), k
        print('%s is reproduced' % OUT)
    else:
        np.savez_compressed(OUT, **arrays)
        print('wrote %s' % OUT)


if __name__ == '__main__':
    main(sys.argv[1:])
