"""tests/golden/next/exact_heaps.npz (tests/golden/make_golden_heaps_exact.py) without a GPU: its shapes, that every
stored minimiser zeroes the float64 gradient of the least-squares cost to rounding, and the cap on the tolerance the
device tests take from it."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = np.finfo(np.float64).eps


def test_fixture_is_consistent_and_its_minimisers_are_stationary():
    z = np.load(os.path.join(HERE, 'golden', 'next', 'exact_heaps.npz'))
    names = [str(n) for n in z['names']]
    sizes = {z['pan_' + n].shape[1] for n in names}
    assert {2, 3, 63, 64, 65, 127, 128, 130, 400, 513} <= sizes
    assert {'exact_rounded', 'flat', 'near_int32_max', 'alpha_above_one', 'far_start', 'misfit_s65', 'misfit_s130',
            'misfit_s400'} <= set(names)
    floors = []
    for n in names:
        pan = z['pan_' + n]
        assert pan.dtype == np.int32 and pan.ndim == 2 and pan.min() >= 1
        for k in ('alpha_', 'kappa_', 'floor_alpha_', 'floor_kappa_'):
            assert z[k + n].dtype == np.float64 and z[k + n].shape == (pan.shape[0],)
        assert (z['steps_' + n] < 200).all()                                  # the restated loop never hit its cap
        floors += [z['floor_alpha_' + n].max(), z['floor_kappa_' + n].max()]
        x = np.arange(1, pan.shape[1] + 1, dtype=np.float64)
        for y, a, k in zip(pan.astype(np.float64), z['alpha_' + n], z['kappa_' + n]):
            p = x ** a
            r = k * p - y
            da, dk = k * p * np.log(x), p
            # rounding of the sums, and of alpha and kappa themselves (half an ulp each, times the curvature)
            slack_a = 8 * EPS * (np.abs(da * r).sum() + (da * da).sum() * abs(a) + abs((da * dk).sum()) * abs(k))
            slack_k = 8 * EPS * (np.abs(dk * r).sum() + (dk * dk).sum() * abs(k) + abs((da * dk).sum()) * abs(a))
            assert abs((da * r).sum()) <= slack_a and abs((dk * r).sum()) <= slack_k, n
    assert z['alpha_flat'][0] == 0.0 and z['kappa_flat'][0] == 777.0
    assert z['pan_near_int32_max'].max() == 2 ** 31 - 1
    assert z['alpha_alpha_above_one'][0] > 1.0
    assert z['pan_far_start'].min() == 3 and z['kappa_far_start'][0] > 1e4
    assert float(z['margin']) == 64.0
    assert float(z['rtol']) == 64.0 * max(floors)
    assert 0.0 < float(z['rtol']) <= 1e-9
