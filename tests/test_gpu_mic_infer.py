"""SIR inference on the device (csrc/mic.hip; include/pgx.h "SIR inference") against the scalar infer_sir, to
which tests/mic_model.py decodes every row. The codes are integers and every comparison the kernel makes is an IEEE
comparison of doubles that the model makes too: the results are equal, not close."""
import itertools

import numpy as np
import pytest

import dev_entry_checks as dev
import mic_model as model
from pangenomix_amd import _native

pytestmark = pytest.mark.gpu

S, R, I, X = 0, 1, 2, 3                                   # the classes; role 0, role 1, and two of role 2
ROLE = {S: 0, R: 1, I: 2, X: 2}
SIR_CODE = {S: 10, R: 11, I: 12, X: 13}
# overlapping ranges: 4.0 is susceptible and intermediate, 8.0 intermediate and resistant, X covers most of them
NUMERIC = {S: ([1.0, 2.0, 4.0], []), I: ([4.0, 8.0], []), R: ([8.0, 16.0], []), X: ([2.0, 3.0, 16.0], [])}
# every route to "needs the host": a class of string MICs alone, a mixed one, one without any MIC
STRINGS = {S: ([], [0, 2]), I: ([4.0, 8.0], [1]), R: ([], []), X: ([2.0, 16.0], [])}
ORDERS = [p for m in range(5) for p in itertools.permutations((S, R, I, X), m)]


def tables(orders, contents):
    """the flattened case tables of pgx_mic_infer: one case per order"""
    class_begin, sir, role, fl_begin, tk_begin, fvals, tvals = [0], [], [], [0], [0], [], []
    for order in orders:
        for c in order:
            sir.append(SIR_CODE[c])
            role.append(ROLE[c])
            fvals += sorted(contents[c][0])
            tvals += sorted(contents[c][1])
            fl_begin.append(len(fvals))
            tk_begin.append(len(tvals))
        class_begin.append(len(sir))
    return (np.array(class_begin, np.uint32), np.array(sir, np.int32), np.array(role, np.uint8), np.array(fl_begin, np.uint32),
            np.array(tk_begin, np.uint32), np.array(fvals, np.float64), np.array(tvals, np.int32))


def edge_values(contents):
    """min and max of every class, one ulp outside each, values between and beyond, NaN and the infinities"""
    out = {0.5, 3.5, 6.0, 12.0, 100.0, float('inf'), float('-inf')}
    for floats, _ in contents.values():
        if floats:
            lo, hi = min(floats), max(floats)
            out |= {lo, hi, float(np.nextafter(lo, -np.inf)), float(np.nextafter(lo, np.inf)), float(np.nextafter(hi, np.inf)),
                    float(np.nextafter(hi, -np.inf))}
    return sorted(out) + [float('nan')]


def rows(n_cases, contents):
    """every case and -1 x every sign code x both combo values x (kind 1 with every edge value, kind 0 with a member
    token, a token of another class, a token of no list and -1, each beside a few values)"""
    values = edge_values(contents)
    keys = [(1, -1, v) for v in values] + [(0, t, v) for t in (-1, 0, 1, 2, 5) for v in (0.5, 4.0, 8.0, 100.0, float('nan'))]
    grid = [(c, s, b) + key for c in list(range(n_cases)) + [-1] for s in (0, 1, 2, 3) for b in (0, 1) for key in keys]
    case, sign, combo, kind, token, value = (np.array(col) for col in zip(*grid))
    return (case.astype(np.int32), sign.astype(np.uint8), combo.astype(np.uint8), kind.astype(np.uint8), token.astype(np.int32),
            value.astype(np.float64))


@pytest.fixture(scope='module')
def numeric():
    t = tables(ORDERS, NUMERIC)
    r = rows(len(ORDERS), NUMERIC)
    return t, r, model.mic_infer(*t, *r)


@pytest.fixture(scope='module')
def strings():
    orders = [p for p in ORDERS if len(p) in (1, 4)]
    t = tables(orders, STRINGS)
    r = rows(len(orders), STRINGS)
    return t, r, model.mic_infer(*t, *r)


def check(ctx, t, r, want):
    got = ctx.mic_infer(*t, *r)
    assert got.dtype == np.int32 and got.shape == want.shape
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, 'rows %r: got %r, want %r; (case, sign, combo, kind, token, value) = %r' % (
        bad[:5].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist(), [tuple(a[bad[0]] for a in r)])
    assert got.tobytes() == ctx.mic_infer(*t, *r).tobytes()
    return got


def test_every_order_of_the_classes_on_numeric_lists(numeric, gpu_ctx):
    t, r, want = numeric
    assert len(ORDERS) == 65 and want.size > 20000
    got = check(gpu_ctx, t, r, want)
    assert set(np.unique(got).tolist()) == {-1, 10, 11, 12, 13}            # no list here sends a row to the host
    case, sign, combo, kind, token, value = r
    # a range hit of an earlier class beats a membership hit of a later one: 8.0 was observed as resistant
    c = ORDERS.index((S, I, R))
    row = np.flatnonzero((case == c) & (sign == 0) & (combo == 0) & (kind == 1) & (value == 8.0))
    assert got[row].tolist() == [SIR_CODE[I]]
    c = ORDERS.index((S, R, I))
    assert got[np.flatnonzero((case == c) & (sign == 0) & (combo == 0) & (kind == 1) & (value == 8.0))].tolist() == [SIR_CODE[R]]
    # with combo set only membership counts: 6.0 lies in a range and was never observed
    assert (got[(combo == 1) & (value == 6.0) & (kind == 1)] == -1).all()
    assert (got[case == -1] == -1).all() and (got[sign == 3] == -1).all() and (got[np.isnan(value) & (kind == 1)] == -1).all()
    assert set(got[sign == 1].tolist()) == {-1, SIR_CODE[S]} and set(got[sign == 2].tolist()) == {-1, SIR_CODE[R]}


def test_one_ulp_outside_a_range(numeric, gpu_ctx):
    t, r, _ = numeric
    only_i = ORDERS.index((I,))
    values = np.array([np.nextafter(4.0, -np.inf), 4.0, 8.0, np.nextafter(8.0, np.inf)])
    n = values.size
    one = (np.full(n, only_i, np.int32), np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.ones(n, np.uint8),
           np.full(n, -1, np.int32), values)
    assert gpu_ctx.mic_infer(*t, *one).tolist() == [-1, 12, 12, -1]
    only_s, only_r = ORDERS.index((S,)), ORDERS.index((R,))
    one = (np.array([only_s] * 2 + [only_r] * 2, np.int32),) + one[1:5] + (np.array([-np.inf, np.nextafter(4.0, np.inf),
                                                                                     np.nextafter(8.0, -np.inf), np.inf]),)
    assert gpu_ctx.mic_infer(*t, *one).tolist() == [10, -1, -1, 11]


def test_lists_with_string_mics_and_every_route_to_the_host(strings, gpu_ctx):
    t, r, want = strings
    got = check(gpu_ctx, t, r, want)
    assert {-2, -1, 10, 12, 13} <= set(np.unique(got).tolist())
    case, sign, combo, kind, token, value = r
    orders = [p for p in ORDERS if len(p) in (1, 4)]
    # strings alone, mixed, empty: each is a route when a range test reaches it; none with combo set
    for cls in (S, I, R):
        c = orders.index((cls,))
        reach = (case == c) & (combo == 0) & (sign == (0 if cls == I else 1 if cls == S else 2)) & (kind == 1) & (value == 100.0)
        assert got[reach].tolist() == [-2], cls
    assert not (got[combo == 1] == -2).any()
    member = (case == orders.index((S,))) & (kind == 0) & (token == 2) & (sign == 0)
    assert (got[member] == SIR_CODE[S]).all() and member.sum() == 10
    assert (got[(kind == 0) & (token == 5) & (combo == 1)] == -1).all()    # a token of no list


@pytest.mark.parametrize('n', (0, 1, 64, 65, 257))
def test_row_counts(n, numeric, gpu_ctx):
    t, r, want = numeric
    pick = np.random.default_rng(n).permutation(want.size)[:n]
    check(gpu_ctx, t, tuple(a[pick] for a in r), want[pick])


def test_invalid_calls_are_refused_before_anything_is_written(numeric, gpu_ctx):
    lib, P, h = _native.lib(), _native._ptr, gpu_ctx._h
    (cb, sir, role, fb, tb, fv, tv), r, _ = numeric
    r = tuple(a[:8].copy() for a in r)
    out = np.full(8, 0x6E6E6E6E, dtype=np.int32)

    def call(cb=cb, n_cases=cb.size - 1, sir=sir, role=role, fb=fb, tb=tb, n_entries=sir.size, fv=fv, n_fvals=fv.size, n_tvals=tv.size,
             n=8):
        return lib.pgx_mic_infer(h, P(cb), n_cases, P(sir), P(role), P(fb), P(tb), n_entries, P(fv), n_fvals, P(tv), n_tvals,
                                 P(r[0]), P(r[1]), P(r[2]), P(r[3]), P(r[4]), P(r[5]), n, P(out))
    bad_fb, bad_role, unsorted, with_nan = fb.copy(), role.copy(), fv.copy(), fv.copy()
    bad_fb[2], bad_role[0], unsorted[:2], with_nan[2] = bad_fb[1] - 1 if bad_fb[1] else 9, 3, unsorted[1::-1], np.nan
    for name, kwargs in (('n', dict(n=1 << 31)), ('cases', dict(n_cases=1 << 24)), ('entries', dict(n_entries=1 << 24)),
                         ('fvals', dict(n_fvals=1 << 24)), ('tvals', dict(n_tvals=1 << 24)), ('fewer entries', dict(n_entries=sir.size - 1)),
                         ('decreasing offsets', dict(fb=bad_fb)), ('a role of 3', dict(role=bad_role)),
                         ('an unsorted run', dict(fv=unsorted)), ('a NaN in a run', dict(fv=with_nan))):
        assert call(**kwargs) == -1, name                 # PGX_ERR_INVALID
        assert (out == 0x6E6E6E6E).all(), name
    assert call() == 0 and not (out == 0x6E6E6E6E).any()
    g = dev.guarded(4096, 0x5A)
    for n, sizes in ((1 << 31, (1, 1, 1, 1)), (8, (1 << 24, 1, 1, 1)), (8, (1, 1 << 24, 1, 1)), (8, (1, 1, 1 << 24, 1)),
                     (8, (1, 1, 1, 1 << 24))):
        with pytest.raises(_native.PgxError) as e:
            gpu_ctx.mic_infer_dev(g.ptr, sizes[0], g.ptr, g.ptr, g.ptr, g.ptr, sizes[1], g.ptr, sizes[2], g.ptr, sizes[3], g.ptr,
                                  g.ptr, g.ptr, g.ptr, g.ptr, g.ptr, n, g.ptr)
        assert e.value.status == -1
    assert g.is_still_garbage()
    g.assert_guards_intact()


# -- the device entry ------------------------------------------------------------------------------------------------------
def run_dev(ctx, t, r, fill, stream):
    n = r[0].size
    with dev.stream_scope(stream) as handle:
        d_t = [dev.upload(a) for a in t]
        d_r = [dev.upload(a) for a in r]
        out = dev.guarded(4 * n, fill)
        with dev.unchanged(*(d for d in d_t + d_r if d.nbytes)):
            ctx.mic_infer_dev(d_t[0].ptr, t[0].size - 1, d_t[1].ptr, d_t[2].ptr, d_t[3].ptr, d_t[4].ptr, t[1].size, d_t[5].ptr,
                              t[5].size, d_t[6].ptr, t[6].size, *[d.ptr for d in d_r], n, out.ptr, handle)
    out.assert_guards_intact()
    return (out.numpy(np.int32),)


@pytest.mark.parametrize('which', ('numeric', 'strings'))
@pytest.mark.parametrize('stream', dev.STREAMS)
def test_device_entry_on_caller_tensors(stream, which, request, gpu_ctx):
    t, r, want = request.getfixturevalue(which)
    pick = np.random.default_rng(3).permutation(want.size)[:3001]
    r, want = tuple(a[pick] for a in r), want[pick]
    per_fill = []
    for fill in dev.FILLS:
        got = run_dev(gpu_ctx, t, r, fill, stream)
        assert np.array_equal(got[0], want)
        per_fill.append(got)
    dev.same_bytes(per_fill)


def test_device_entry_does_not_allocate(numeric, gpu_ctx):
    t, r, want = numeric
    r = tuple(a[:5000] for a in r)
    d_t, d_r = [dev.upload(a) for a in t], [dev.upload(a) for a in r]
    out = dev.guarded(4 * 5000, 0xFF)
    dev.assert_no_allocation(lambda: gpu_ctx.mic_infer_dev(
        d_t[0].ptr, t[0].size - 1, d_t[1].ptr, d_t[2].ptr, d_t[3].ptr, d_t[4].ptr, t[1].size, d_t[5].ptr, t[5].size, d_t[6].ptr,
        t[6].size, *[d.ptr for d in d_r], 5000, out.ptr))
    assert np.array_equal(out.numpy(np.int32), want[:5000])
