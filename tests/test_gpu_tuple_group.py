"""Exact grouping of int32 tuples on the device (csrc/mic.hip; include/pgx.h "Exact grouping of fixed-width integer tuples";
DESIGN.md 6o) against a dict over the rows (tests/mic_model.py). Integers: every comparison is exact, and every call is made
twice for the same bytes."""
import numpy as np
import pytest

import dev_entry_checks as dev
import mic_model as model
from pangenomix_amd import _native

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 4099)
KS = (1, 2, 7, 8)
EDGES = np.array([-2 ** 31, -1, 0, 2 ** 31 - 1], dtype=np.int64)


def check(ctx, cols, flags=0):
    cols = np.ascontiguousarray(cols, dtype=np.int32)
    want = model.tuple_group(cols)
    got = ctx.tuple_group(cols, flags)
    assert got[0].dtype == np.int32 and got[1].dtype == np.uint32
    assert np.array_equal(got[0], want[0]), 'first differs at %r' % np.flatnonzero(got[0] != want[0])[:10].tolist()
    assert np.array_equal(got[1], want[1]), 'count differs at %r' % np.flatnonzero(got[1] != want[1])[:10].tolist()
    assert got[2] == want[2]
    again = ctx.tuple_group(cols, flags)
    assert got[0].tobytes() == again[0].tobytes() and got[1].tobytes() == again[1].tobytes() and got[2] == again[2]
    n = cols.shape[1]
    off = got[0] != np.arange(n)
    assert not got[1][off].any() and int(got[1].sum()) == n and (got[1][~off] >= 1).all()     # count is zero off the representatives
    return got


def heavy_tailed(rng, n, k, distinct):
    """records drawn from `distinct` tuples with multiplicities ~ 1 / rank"""
    pool = rng.integers(-5, 6, (k, max(distinct, 1)))
    pool[0] = np.arange(pool.shape[1])                    # (distinct for certain)
    p = 1.0 / np.arange(1, pool.shape[1] + 1)
    return pool[:, rng.choice(pool.shape[1], n, p=p / p.sum())].astype(np.int32)


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('n', SIZES)
def test_sizes_and_widths(n, k, gpu_ctx):
    rng = np.random.default_rng(1000 * n + k)
    got = check(gpu_ctx, heavy_tailed(rng, n, k, 40))
    if n >= 255:
        assert 1 < got[2] <= 40 and got[1].max() > n // 10
    check(gpu_ctx, np.full((k, n), 7))                    # all records equal: every lane of every wave at one slot
    check(gpu_ctx, rng.permutation(n)[None, :].repeat(k, axis=0) if n else np.zeros((k, 0)))   # all distinct


@pytest.mark.parametrize('k', (2, 7, 8))
def test_tuples_that_differ_in_one_column_only(k, gpu_ctx):
    n = 777
    rng = np.random.default_rng(k)
    for col in (0, k - 1):
        cols = np.full((k, n), 3, dtype=np.int32)
        cols[col] = rng.integers(0, 9, n)
        got = check(gpu_ctx, cols)
        assert got[2] == 9
    cols = np.full((k, n), 3, dtype=np.int32)             # the same values in another column are another tuple
    cols[0, ::2], cols[k - 1, 1::2] = 5, 5
    assert check(gpu_ctx, cols)[2] == 2


@pytest.mark.parametrize('k', KS)
def test_extreme_values(k, gpu_ctx):
    rng = np.random.default_rng(77 + k)
    cols = EDGES[rng.integers(0, 4, (k, 1500))]
    got = check(gpu_ctx, cols)
    assert got[2] == min(4 ** k, len({tuple(c) for c in cols.T.tolist()}))
    grid = np.array(np.meshgrid(*[EDGES] * min(k, 2), indexing='ij')).reshape(min(k, 2), -1)
    check(gpu_ctx, np.concatenate([grid, grid[:, ::-1]], axis=1))


def test_heavy_tailed_multiplicities(gpu_ctx):
    rng = np.random.default_rng(9)
    got = check(gpu_ctx, heavy_tailed(rng, 20000, 7, 3000))
    assert got[2] > 1000 and got[1].max() > 1500
    # a table's shape: long runs of one tuple, then a sprinkle of rare ones
    cols = np.repeat(heavy_tailed(rng, 300, 3, 30), 50, axis=1)
    cols[:, rng.integers(0, cols.shape[1], 500)] = rng.integers(100, 200, (3, 500))
    check(gpu_ctx, cols)


@pytest.mark.parametrize('k', (1, 7))
def test_narrow_hash_gives_the_same_results(k, gpu_ctx):
    rng = np.random.default_rng(300 + k)
    cols = heavy_tailed(rng, 2000, k, 300)
    wide = check(gpu_ctx, cols)
    narrow = check(gpu_ctx, cols, _native.TUPLE_NARROW_HASH)
    assert 250 <= wide[2] <= 300
    assert all(a.tobytes() == b.tobytes() for a, b in zip(wide[:2], narrow[:2])) and wide[2] == narrow[2]


def test_invalid_calls_are_refused_before_anything_is_written(gpu_ctx):
    lib, P, h = _native.lib(), _native._ptr, gpu_ctx._h
    cols = np.arange(16, dtype=np.int32).reshape(2, 8)
    first, count, distinct = np.full(8, 0x6E6E6E6E, np.int32), np.full(8, 0x6E6E6E6E, np.uint32), np.full(1, 0x6E6E6E6E, np.uint32)

    def call(n=8, k=2, flags=0):
        return lib.pgx_tuple_group(h, P(cols), n, k, flags, P(first), P(count), P(distinct))
    for kwargs in (dict(k=0), dict(k=9), dict(n=1 << 24), dict(flags=2)):
        assert call(**kwargs) == -1, kwargs               # PGX_ERR_INVALID
        assert (first == 0x6E6E6E6E).all() and (count == 0x6E6E6E6E).all() and distinct[0] == 0x6E6E6E6E, kwargs
    assert call() == 0 and first.tolist() == list(range(8)) and count.tolist() == [1] * 8 and distinct[0] == 8
    assert call(n=0) == 0 and distinct[0] == 0
    wsb = gpu_ctx.tuple_group_workspace_bytes
    assert wsb(1 << 24, 2) == 0 and wsb(8, 0) == 0 and wsb(8, 9) == 0 and wsb(8, 2) > 0 and wsb(0, 1) > 0
    need = wsb(8, 2)
    g = dev.guarded(4096 + need, 0x5A)
    for n, k, flags, ws_bytes in ((8, 0, 0, need), (8, 9, 0, need), (1 << 24, 2, 0, need), (8, 2, 2, need), (8, 2, 0, need - 1)):
        with pytest.raises(_native.PgxError) as e:
            gpu_ctx.tuple_group_dev(g.ptr, n, k, g.ptr, g.ptr, g.ptr, g.ptr + 4096, ws_bytes, flags)
        assert e.value.status == -1
    assert g.is_still_garbage()
    g.assert_guards_intact()


# -- the device entry ------------------------------------------------------------------------------------------------------
def run_dev(ctx, cols, flags, fill, stream):
    k, n = cols.shape
    need = ctx.tuple_group_workspace_bytes(n, k)
    with dev.stream_scope(stream) as handle:
        d_cols = dev.upload(cols)
        first, count, distinct, ws = dev.guarded(4 * n, fill), dev.guarded(4 * n, fill), dev.guarded(4, fill), dev.guarded(need, fill)
        with dev.unchanged(d_cols):
            ctx.tuple_group_dev(d_cols.ptr, n, k, first.ptr, count.ptr, distinct.ptr, ws.ptr, need, flags, handle)
    for g in (first, count, distinct, ws):
        g.assert_guards_intact()
    return first.numpy(np.int32), count.numpy(np.uint32), distinct.numpy(np.uint32)


@pytest.mark.parametrize('flags', (0, _native.TUPLE_NARROW_HASH))
@pytest.mark.parametrize('stream', dev.STREAMS)
def test_device_entry_on_caller_tensors(stream, flags, gpu_ctx):
    rng = np.random.default_rng(5)
    for n, k, distinct in ((1500, 7, 200), (1, 1, 1), (65, 8, 3)):
        cols = heavy_tailed(rng, n, k, distinct)
        want = model.tuple_group(cols)
        per_fill = []
        for fill in dev.FILLS:
            got = run_dev(gpu_ctx, cols, flags, fill, stream)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2][0] == want[2]
            per_fill.append(got)
        dev.same_bytes(per_fill)


def test_device_entry_with_no_records_and_without_allocation(gpu_ctx):
    distinct = dev.guarded(4, 0xFF)
    gpu_ctx.tuple_group_dev(None, 0, 3, None, None, distinct.ptr, None, 0)
    assert distinct.numpy(np.uint32)[0] == 0
    cols = heavy_tailed(np.random.default_rng(6), 3000, 7, 500)
    need = gpu_ctx.tuple_group_workspace_bytes(3000, 7)
    d_cols = dev.upload(cols)
    first, count, ws = dev.guarded(4 * 3000, 0xFF), dev.guarded(4 * 3000, 0xFF), dev.guarded(need, 0xFF)
    dev.assert_no_allocation(lambda: gpu_ctx.tuple_group_dev(d_cols.ptr, 3000, 7, first.ptr, count.ptr, distinct.ptr, ws.ptr, need))
    assert np.array_equal(first.numpy(np.int32), model.tuple_group(cols)[0])
