"""The device-pointer entry points (pgx_*_dev) as a PyTorch-ROCm program uses them: raw addresses of caller tensors, a
caller workspace of exactly pgx_*_workspace_bytes() bytes, a caller stream. Every output buffer and workspace sits
between guard bands and is full of garbage (two patterns; both must give the same bytes), inputs are made on the stream
right before the call and must come back unchanged, each entry runs on stream 0 and on a side stream, and an entry that
promises not to allocate is held to it (tests/dev_entry_checks.py).

References are never the code under test: numpy, the CPU oracle, the fixtures the reference itself produced
(tests/golden/core, tests/golden/betabinom), the exact Heaps minimisers of tests/golden/next/exact_heaps.npz. Integer
results are compared bit for bit. Equality with the host-pointer entries is asserted in addition."""
import os

import numpy as np
import pytest
import torch

import dev_entry_checks as chk
import oracle
import test_betabinom_host as host
import test_gpu_bernoulli
import test_gpu_cluster
from oracle import heaps_ref
from pangenomix_amd import _native, synth
from pangenomix_amd import pangenome_analysis as pa
from test_cluster_oracle import AA as AA_LETTERS, nt_params, pack, params, rand_nt, rand_seq, revcomp

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def stride_words(n_rows):
    return int(_native.lib().pgx_bitmap_stride_words(int(n_rows)))


def bitmap_reference(row, col, S, stride):
    """genome-major, gene g = bit g & 63 of word g >> 6 (pgx.h), from a dense table packed by numpy; pad bits zero"""
    dense = np.zeros((S, stride * 64), dtype=bool)
    dense[np.asarray(col, dtype=np.int64), np.asarray(row, dtype=np.int64)] = True
    return np.packbits(dense, axis=1, bitorder='little').view('<u8').astype(np.uint64)


def random_coo(rng, G, S, density, full_rows=0):
    """Distinct coordinates of a G x S table, about `density` of its cells, plus `full_rows` rows present everywhere
    (so that the core curves do not fall to zero at once); never empty."""
    n = max(1, int(G * S * density))
    keys = np.unique(np.concatenate((rng.integers(0, G * S, size=n), [0])))
    if full_rows:
        full = (rng.choice(G, size=min(full_rows, G), replace=False)[:, None] * S + np.arange(S)[None, :]).reshape(-1)
        keys = np.unique(np.concatenate((keys, full)))
    return (keys // S).astype(np.int32), (keys % S).astype(np.int32)


# ---- pgx_presence_bitmap_dev ------------------------------------------------------------------------------------------
def run_presence(ctx, kind, fill, rows, cols, G, S, with_counters=True):
    stride = stride_words(G)
    with chk.stream_scope(kind) as st:
        bits = chk.guarded(S * stride * 8, fill)
        cnt = chk.guarded(16, fill) if with_counters else None
        d_r, d_c = chk.upload(rows), chk.upload(cols)
        with chk.unchanged(d_r, d_c):
            ctx.presence_bitmap_dev(d_r.ptr, d_c.ptr, rows.size, G, S, bits.ptr, st, cnt.ptr if cnt else None)
    bits.assert_guards_intact()
    if cnt:
        cnt.assert_guards_intact()
    return (bits.numpy(np.uint64).reshape(S, stride),) + ((cnt.numpy(np.uint64),) if cnt else ())


@pytest.mark.parametrize('S', [1, 3, 65])
@pytest.mark.parametrize('G', [1, 63, 64, 65, 1024, 1025, 70001])
@pytest.mark.parametrize('kind', chk.STREAMS)
def test_presence_bitmap_dev_counts_and_skips(G, S, kind, gpu_ctx):
    """Valid records, five of them twice, and six records out of range (negative values, row == n_rows, genome ==
    n_genomes, INT32_MIN, INT32_MAX), shuffled: the bitmap is the one of the valid records alone with pad bits zero,
    d_counters = {5 or fewer duplicates, 6}. G = 70001 x S = 65 has more than 4096 x 256 records (the grid-stride loop)."""
    rng = np.random.default_rng(G * 131 + S)
    row, col = random_coo(rng, G, S, 0.3)
    n_dup = min(5, row.size)
    again = rng.choice(row.size, size=n_dup, replace=False)
    bad_r = np.array([-1, 0, G, 0, INT32_MIN, INT32_MAX], dtype=np.int32)
    bad_c = np.array([0, -1, 0, S, 0, INT32_MAX], dtype=np.int32)
    order = rng.permutation(row.size + n_dup + bad_r.size)
    rows = np.concatenate((row, row[again], bad_r))[order]
    cols = np.concatenate((col, col[again], bad_c))[order]
    if (G, S) == (70001, 65):
        assert rows.size > 4096 * 256
    got = chk.same_bytes([run_presence(gpu_ctx, kind, f, rows, cols, G, S) for f in chk.FILLS])
    want = bitmap_reference(row, col, S, stride_words(G))
    assert np.array_equal(got[0], want)
    assert got[1].tolist() == [n_dup, bad_r.size]
    assert np.array_equal(got[0], gpu_ctx.presence_bitmap(row, col, G, S))        # in addition: the host entry


@pytest.mark.parametrize('kind', chk.STREAMS)
def test_presence_bitmap_dev_without_counters_and_without_records(kind, gpu_ctx):
    rng = np.random.default_rng(3)
    G, S = 1025, 7
    row, col = random_coo(rng, G, S, 0.4)
    rows, cols = np.concatenate((row, [G, 5])).astype(np.int32), np.concatenate((col, [0, S])).astype(np.int32)
    got = chk.same_bytes([run_presence(gpu_ctx, kind, f, rows, cols, G, S, with_counters=False) for f in chk.FILLS])
    assert np.array_equal(got[0], bitmap_reference(row, col, S, stride_words(G)))
    clean = chk.same_bytes([run_presence(gpu_ctx, kind, f, row, col, G, S) for f in chk.FILLS])
    assert np.array_equal(clean[0], got[0]) and clean[1].tolist() == [0, 0]
    # no records at all: the all-ones bitmap and the counters are zeroed, NULL record arrays are accepted
    empty = np.zeros(0, np.int32)
    none = chk.same_bytes([run_presence(gpu_ctx, kind, f, empty, empty, G, S) for f in chk.FILLS])
    assert not none[0].any() and none[1].tolist() == [0, 0]


def test_presence_bitmap_dev_does_not_allocate(gpu_ctx):
    rng = np.random.default_rng(4)
    G, S = 5000, 33
    row, col = random_coo(rng, G, S, 0.2)
    bits, cnt = chk.guarded(S * stride_words(G) * 8, 0xFF), chk.guarded(16, 0xFF)
    d_r, d_c = chk.upload(row), chk.upload(col)
    chk.assert_no_allocation(lambda: gpu_ctx.presence_bitmap_dev(d_r.ptr, d_c.ptr, row.size, G, S, bits.ptr, 0, cnt.ptr))
    assert np.array_equal(bits.numpy(np.uint64).reshape(S, -1), bitmap_reference(row, col, S, stride_words(G)))


# ---- pgx_row_counts_dev -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_genomes', [0, 1, 400])
@pytest.mark.parametrize('n_rows', [1, 255, 256, 257, 70001])
@pytest.mark.parametrize('kind', chk.STREAMS)
def test_row_counts_dev(n_rows, n_genomes, kind, gpu_ctx):
    rng = np.random.default_rng(n_rows * 7 + n_genomes)
    stride = stride_words(n_rows)
    if n_genomes:
        row, col = random_coo(rng, n_rows, n_genomes, 0.3, full_rows=2)
        bits = bitmap_reference(row, col, n_genomes, stride)
        want = np.bincount(row, minlength=n_rows).astype(np.int32)
    else:
        bits = np.full((1, stride), ~np.uint64(0))          # (never read: no genome owns it)
        want = np.zeros(n_rows, dtype=np.int32)

    def run(fill):
        with chk.stream_scope(kind) as st:
            counts = chk.guarded(n_rows * 4, fill)
            d_bits = chk.upload(bits)
            with chk.unchanged(d_bits):
                gpu_ctx.row_counts_dev(d_bits.ptr, n_rows, n_genomes, counts.ptr, st)
        counts.assert_guards_intact()
        return (counts.numpy(np.int32),)

    got = chk.same_bytes([run(f) for f in chk.FILLS])
    assert np.array_equal(got[0], want)
    if n_genomes:
        assert np.array_equal(gpu_ctx.row_counts(row, col, n_rows, n_genomes)[0], want)


def test_row_counts_dev_without_rows_and_without_allocation(gpu_ctx):
    gpu_ctx.row_counts_dev(None, 0, 5, None, 0)                                  # n_rows = 0: nothing to do, NULL accepted
    rng = np.random.default_rng(9)
    row, col = random_coo(rng, 3000, 40, 0.3)
    d_bits = chk.upload(bitmap_reference(row, col, 40, stride_words(3000)))
    counts = chk.guarded(3000 * 4, 0xFF)
    chk.assert_no_allocation(lambda: gpu_ctx.row_counts_dev(d_bits.ptr, 3000, 40, counts.ptr, 0))
    assert np.array_equal(counts.numpy(np.int32), np.bincount(row, minlength=3000))


# ---- pgx_pan_core_dev -------------------------------------------------------------------------------------------------
PAN_S = [1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 513]
PAN_SHAPES = [(G, S, (1, 3, 4, 5)[(i + j) % 4]) for j, G in enumerate((300, 70001)) for i, S in enumerate(PAN_S)]
PAN_SHAPES += [(150000, 400, 1), (150000, 700, 1)]         # the same G on both sides of the sweep's 3 MiB L2 rule
# (n_iter is rotated over the shapes, not crossed with S: every (G, S) meets one n_iter, and S = 63, 64, 65 meet the
# four-iterations-per-workgroup packing -- n_iter 3, 4, 5 -- through that rotation only)


def pan_ws_bytes(G, S, n_iter):
    return int(_native.lib().pgx_pan_core_workspace_bytes(G, S, n_iter))


def pan_partials(G, S, n_iter):
    nws = pan_ws_bytes(G, S, n_iter)
    assert nws % (4 * n_iter * S) == 0
    return nws // (4 * n_iter * S)


def test_pan_core_shapes_cover_the_sweeps_geometries():
    """The number of partial sums per output (stripes x waves per stripe) follows from the workspace size. The shapes
    below must produce at least three different ones, more than one wave per stripe among them, and one pair with the
    same G whose stripe count differs because n_genomes x stripe bytes crossed 3 MiB (150,000 genes: 4 stripes x 5 waves
    up to 668 genomes, 8 x 3 beyond)."""
    partials = {shape: pan_partials(*shape) for shape in PAN_SHAPES}
    assert len(set(partials.values())) >= 3
    assert partials[(150000, 400, 1)] == 20 and partials[(150000, 700, 1)] == 24
    assert any(G == 70001 and p > 8 for (G, S, n), p in partials.items())        # at most 8 stripes: several waves in each


def run_pan_core(ctx, kind, fill, bits, G, S, perms):
    n_iter = perms.shape[0]
    nws = pan_ws_bytes(G, S, n_iter)
    with chk.stream_scope(kind) as st:
        pan, core, ws = chk.guarded(n_iter * S * 4, fill), chk.guarded(n_iter * S * 4, fill), chk.guarded(nws, fill)
        d_bits, d_perms = chk.upload(bits), chk.upload(perms)
        with chk.unchanged(d_bits, d_perms):
            ctx.pan_core_dev(d_bits.ptr, G, S, d_perms.ptr, n_iter, pan.ptr, core.ptr, ws.ptr, nws, st)
    for b in (pan, core, ws):
        b.assert_guards_intact()
    return pan.numpy(np.int32).reshape(n_iter, S), core.numpy(np.int32).reshape(n_iter, S)


@pytest.mark.parametrize('G,S,n_iter', PAN_SHAPES)
@pytest.mark.parametrize('kind', chk.STREAMS)
def test_pan_core_dev_matches_the_oracle(G, S, n_iter, kind, gpu_ctx):
    rng = np.random.default_rng(G + 31 * S + n_iter)
    n_full = min(G // 10 + 1, 2000)
    row, col = random_coo(rng, G, S, 0.02 if G > 100000 else 0.2, full_rows=n_full)
    perms = np.array([rng.permutation(S) for _ in range(n_iter)], dtype=np.int32)
    bits = bitmap_reference(row, col, S, stride_words(G))
    pan, core = chk.same_bytes([run_pan_core(gpu_ctx, kind, f, bits, G, S, perms) for f in chk.FILLS])
    opan, ocore = oracle.pan_core(row, col, None, G, S, perms)
    assert np.array_equal(pan, opan) and np.array_equal(core, ocore)
    assert core[:, -1].min() >= n_full                                            # (the core curves are not trivially zero)


def test_pan_core_dev_refusals_and_no_allocation(gpu_ctx):
    rng = np.random.default_rng(12)
    G, S, n_iter = 9000, 37, 3
    row, col = random_coo(rng, G, S, 0.2, full_rows=50)
    perms = np.array([rng.permutation(S) for _ in range(n_iter)], dtype=np.int32)
    nws = pan_ws_bytes(G, S, n_iter)
    # (the bitmap with 16 spare bytes behind it, for the address that is off by 8)
    d_bits = chk.upload(np.concatenate((bitmap_reference(row, col, S, stride_words(G)).reshape(-1), np.zeros(2, np.uint64))))
    d_perms = chk.upload(perms)
    pan, core, ws = chk.guarded(n_iter * S * 4, 0xFF), chk.guarded(n_iter * S * 4, 0xFF), chk.guarded(nws, 0xFF)
    args = (G, S, d_perms.ptr, n_iter, pan.ptr, core.ptr, ws.ptr)
    with pytest.raises(_native.PgxError, match='workspace too small'):
        gpu_ctx.pan_core_dev(d_bits.ptr, *args, nws - 1, 0)
    with pytest.raises(_native.PgxError, match='16-byte aligned'):
        gpu_ctx.pan_core_dev(d_bits.ptr + 8, *args, nws, 0)
    gpu_ctx.pan_core_dev(d_bits.ptr, G, S, d_perms.ptr, 0, pan.ptr, core.ptr, ws.ptr, 0, 0)     # n_iter = 0: nothing to do
    torch.cuda.synchronize()
    assert pan.is_still_garbage() and core.is_still_garbage() and ws.is_still_garbage()
    chk.assert_no_allocation(lambda: gpu_ctx.pan_core_dev(d_bits.ptr, *args, nws, 0))
    opan, ocore = oracle.pan_core(row, col, None, G, S, perms)
    assert np.array_equal(pan.numpy(np.int32).reshape(n_iter, S), opan)
    assert np.array_equal(core.numpy(np.int32).reshape(n_iter, S), ocore)
    for b in (pan, core, ws):
        b.assert_guards_intact()


# ---- pgx_heaps_fit_dev ------------------------------------------------------------------------------------------------
def run_heaps(ctx, kind, fill, table):
    n_iter, S = table.shape
    with chk.stream_scope(kind) as st:
        alpha, kappa = chk.guarded(n_iter * 8, fill), chk.guarded(n_iter * 8, fill)
        d_pan = chk.upload(table.astype(np.int32))
        with chk.unchanged(d_pan):
            ctx.heaps_fit_dev(d_pan.ptr, n_iter, S, alpha.ptr, kappa.ptr, st)
    alpha.assert_guards_intact(), kappa.assert_guards_intact()
    return alpha.numpy(np.float64), kappa.numpy(np.float64)


@pytest.mark.parametrize('n_iter', [1, 3, 4, 5, 1000])
@pytest.mark.parametrize('kind', chk.STREAMS)
def test_heaps_fit_dev_equals_the_float64_entry_bit_for_bit(n_iter, kind, gpu_ctx):
    """The int32 instantiation differs from the float64 one in (double)y[j] alone. Independent of both: scipy's fit of a
    sample of the rows, at the tolerance the scipy-based tests use (scipy stops ~3e-6 from the minimum)."""
    rng = np.random.default_rng(n_iter)
    S = 129
    x = np.arange(1, S + 1)
    table = np.maximum.accumulate(np.rint(rng.uniform(500, 5000, (n_iter, 1)) * x ** rng.uniform(0.2, 0.7, (n_iter, 1))
                                          * (1 + 0.01 * rng.standard_normal((n_iter, S)))), axis=1).astype(np.int32)
    alpha, kappa = chk.same_bytes([run_heaps(gpu_ctx, kind, f, table) for f in chk.FILLS])
    ha, hk = gpu_ctx.heaps_fit(table.astype(np.float64))
    assert alpha.tobytes() == ha.tobytes() and kappa.tobytes() == hk.tobytes()
    sample = sorted({0, n_iter // 2, n_iter - 1})
    oa, ok = heaps_ref.fit_rows(table[sample])
    np.testing.assert_allclose(alpha[sample], oa, rtol=1e-5)
    np.testing.assert_allclose(kappa[sample], ok, rtol=1e-5)


def heaps_exact():
    return np.load(os.path.join(HERE, 'golden', 'next', 'exact_heaps.npz'))


def assert_exact_fit(name, alpha, kappa, z, what):
    """alpha relative to the exact minimiser (absolute where it is 0), kappa relative; every figure is printed first."""
    rtol = float(z['rtol'])
    wa, wk = z['alpha_' + name], z['kappa_' + name]
    ea = np.abs(alpha - wa) / np.where(wa == 0, 1.0, np.abs(wa))
    ek = np.abs(kappa - wk) / np.abs(wk)
    print('heaps_exact %-16s %-8s err alpha %s  err kappa %s  (rtol %.3e)'
          % (name, what, ' '.join('%.2e' % e for e in ea), ' '.join('%.2e' % e for e in ek), rtol))
    assert (ea <= rtol).all() and (ek <= rtol).all(), (name, what, ea.max(), ek.max(), rtol)


@pytest.mark.parametrize('name', [str(n) for n in heaps_exact()['names']])
def test_heaps_fit_against_the_exact_minimisers(name, gpu_ctx):
    """Both instantiations against the 60-digit least-squares minimisers of tests/golden/next/exact_heaps.npz
    (tests/golden/make_golden_heaps_exact.py). Tolerance: the fixture's `rtol` = 64 x the largest distance a float64
    numpy restatement of the kernel's fit, in four rounding variants, ends from those minimisers on the CPU
    = 64 x 9.93e-16 = 6.4e-14 (the generator's RTOL_CAP: 1e-9); it was measured on the restatement, not on the device.
    The misfit_* rows have residuals of per cents: there a Jacobian term that is off by 1e-7 moves the fit by 1e-11 to
    1e-9, which rows that a power law fits well do not show."""
    z = heaps_exact()
    table = z['pan_' + name]
    assert float(z['rtol']) <= 1e-9
    for kind in chk.STREAMS:
        alpha, kappa = chk.same_bytes([run_heaps(gpu_ctx, kind, f, table) for f in chk.FILLS])
        assert_exact_fit(name, alpha, kappa, z, 'int32/' + kind)
    ha, hk = gpu_ctx.heaps_fit(table.astype(np.float64))
    assert_exact_fit(name, ha, hk, z, 'float64')
    assert ha.tobytes() == alpha.tobytes() and hk.tobytes() == kappa.tobytes()


def test_heaps_fit_dev_in_place_on_pan_core_devs_output(gpu_ctx):
    """The use pgx.h advertises: the curves of pgx_pan_core_dev are fitted where they lie, on the same side stream, with
    no host synchronisation in between; and the fit does not allocate."""
    rng = np.random.default_rng(21)
    G, S, n_iter = 20000, 130, 5
    row, col = random_coo(rng, G, S, 0.05, full_rows=100)
    perms = np.array([rng.permutation(S) for _ in range(n_iter)], dtype=np.int32)
    bits = bitmap_reference(row, col, S, stride_words(G))
    nws = pan_ws_bytes(G, S, n_iter)

    def run(fill):
        with chk.stream_scope('side') as st:
            pan, core, ws = chk.guarded(n_iter * S * 4, fill), chk.guarded(n_iter * S * 4, fill), chk.guarded(nws, fill)
            alpha, kappa = chk.guarded(n_iter * 8, fill), chk.guarded(n_iter * 8, fill)
            d_bits, d_perms = chk.upload(bits), chk.upload(perms)
            gpu_ctx.pan_core_dev(d_bits.ptr, G, S, d_perms.ptr, n_iter, pan.ptr, core.ptr, ws.ptr, nws, st)
            gpu_ctx.heaps_fit_dev(pan.ptr, n_iter, S, alpha.ptr, kappa.ptr, st)
        for b in (pan, core, ws, alpha, kappa):
            b.assert_guards_intact()
        return pan.numpy(np.int32).reshape(n_iter, S), alpha.numpy(np.float64), kappa.numpy(np.float64)

    pan, alpha, kappa = chk.same_bytes([run(f) for f in chk.FILLS])
    opan, _ = oracle.pan_core(row, col, None, G, S, perms)
    assert np.array_equal(pan, opan)
    oa, ok = heaps_ref.fit_rows(opan)
    np.testing.assert_allclose(alpha, oa, rtol=1e-5)
    np.testing.assert_allclose(kappa, ok, rtol=1e-5)
    ha, hk = gpu_ctx.heaps_fit(opan.astype(np.float64))
    assert alpha.tobytes() == ha.tobytes() and kappa.tobytes() == hk.tobytes()
    d_pan, a, k = chk.upload(opan), chk.guarded(n_iter * 8, 0xFF), chk.guarded(n_iter * 8, 0xFF)
    chk.assert_no_allocation(lambda: gpu_ctx.heaps_fit_dev(d_pan.ptr, n_iter, S, a.ptr, k.ptr, 0))
    gpu_ctx.heaps_fit_dev(None, 0, S, None, None, 0)                              # n_iter = 0: nothing to do


# ---- pgx_bernoulli_eval_dev -------------------------------------------------------------------------------------------
def bern_ws_bytes(G, S):
    return int(_native.lib().pgx_bernoulli_workspace_bytes(G, S))


def run_bernoulli(ctx, kind, fill, rows, cols, G, S, pq, flags):
    """The bitmap is made by pgx_presence_bitmap_dev on the same stream (NULL when the table has no cell)."""
    nws = bern_ws_bytes(G, S)
    with chk.stream_scope(kind) as st:
        out, ws = chk.guarded((1 + G + S) * 8, fill), chk.guarded(nws, fill)
        d_pq = chk.upload(pq)
        bits = None
        if G and S:
            bits = chk.guarded(S * stride_words(G) * 8, fill)
            d_r, d_c = chk.upload(rows), chk.upload(cols)
            ctx.presence_bitmap_dev(d_r.ptr, d_c.ptr, rows.size, G, S, bits.ptr, st)
        with chk.unchanged(*([d_pq] + ([bits.raw] if bits else []))):
            ctx.bernoulli_eval_dev(bits.ptr if bits else None, G, S, d_pq.ptr, out.ptr, ws.ptr, nws, flags, st)
    out.assert_guards_intact(), ws.assert_guards_intact()
    return (out.numpy(np.float64),)


@pytest.mark.parametrize('path', test_gpu_bernoulli.CASES, ids=test_gpu_bernoulli.IDS)
def test_bernoulli_eval_dev_matches_the_reference(path, gpu_ctx):
    z = np.load(path)
    G, S = (int(v) for v in z['shape'])
    rows, cols = z['rows'].astype(np.int32), z['cols'].astype(np.int32)
    assert gpu_ctx.bernoulli_load(rows, cols, G, S) == 0
    for k, pt in enumerate(z['points']):
        for flags in (0, 1):
            for kind in chk.STREAMS:
                out, = chk.same_bytes([run_bernoulli(gpu_ctx, kind, f, rows, cols, G, S, pt, flags) for f in chk.FILLS])
                test_gpu_bernoulli.assert_evaluation(out, z['point_ll'][k], z['point_grad'][k], z['point_scale'][k])
                assert out.tobytes() == gpu_ctx.bernoulli_eval(pt, exact=bool(flags)).tobytes()


@pytest.mark.parametrize('G,S', [(300, 0), (0, 7), (0, 0)])
@pytest.mark.parametrize('kind', chk.STREAMS)
def test_bernoulli_eval_dev_of_an_empty_table(G, S, kind, gpu_ctx):
    """No cell: LL = 0 and every gradient entry 0 (0 / p - 0), d_bits = NULL, whatever the workspace held."""
    pq = np.linspace(0.3, 0.9, G + S) if G + S else np.zeros(1)
    empty = np.zeros(0, np.int32)
    for flags in (0, 1):
        out, = chk.same_bytes([run_bernoulli(gpu_ctx, kind, f, empty, empty, G, S, pq, flags) for f in chk.FILLS])
        assert out.shape == (1 + G + S,) and not out.any() and not np.signbit(out[0])


def test_bernoulli_eval_dev_refusals_and_no_allocation(gpu_ctx):
    z = np.load([p for p in test_gpu_bernoulli.CASES if 'g128' in p][0])
    G, S = (int(v) for v in z['shape'])
    nws = bern_ws_bytes(G, S)
    d_bits = chk.upload(bitmap_reference(z['rows'], z['cols'], S, stride_words(G)))
    d_pq = chk.upload(z['points'][0])
    out, ws = chk.guarded((1 + G + S) * 8, 0xFF), chk.guarded(nws, 0xFF)
    with pytest.raises(_native.PgxError, match='unknown flag'):
        gpu_ctx.bernoulli_eval_dev(d_bits.ptr, G, S, d_pq.ptr, out.ptr, ws.ptr, nws, 2, 0)
    with pytest.raises(_native.PgxError, match='workspace too small'):
        gpu_ctx.bernoulli_eval_dev(d_bits.ptr, G, S, d_pq.ptr, out.ptr, ws.ptr, nws - 1, 0, 0)
    torch.cuda.synchronize()
    assert out.is_still_garbage() and ws.is_still_garbage()
    chk.assert_no_allocation(lambda: gpu_ctx.bernoulli_eval_dev(d_bits.ptr, G, S, d_pq.ptr, out.ptr, ws.ptr, nws, 0, 0))
    test_gpu_bernoulli.assert_evaluation(out.numpy(np.float64), z['point_ll'][0], z['point_grad'][0], z['point_scale'][0])
    out.assert_guards_intact(), ws.assert_guards_intact()


# ---- pgx_bbn_ks_sim_dev -----------------------------------------------------------------------------------------------
def run_bbn(ctx, kind, fill, words, cdf, model_cdf, n_samples, iterations):
    L = cdf.size
    nws = int(_native.lib().pgx_bbn_workspace_bytes(L, iterations))
    assert (nws == 0) == (L <= 4096 or iterations == 0)
    with chk.stream_scope(kind) as st:
        ks, ws = chk.guarded(iterations * 8, fill), chk.guarded(nws, fill)
        d_w, d_cdf, d_model = chk.upload(words), chk.upload(cdf), chk.upload(model_cdf)
        with chk.unchanged(d_w, d_cdf, d_model):
            ctx.bbn_ks_sim_dev(d_w.ptr, d_cdf.ptr, d_model.ptr, L, n_samples, iterations, ks.ptr, ws.ptr, nws, st)
    ks.assert_guards_intact(), ws.assert_guards_intact()
    return (ks.numpy(np.float64),)


def bbn_inputs(n, a, b, L, n_samples, iterations):
    """cdfs as ks_montecarlo_bbn makes them, and the words of numpy's legacy generator from its CURRENT state"""
    model_cdf = np.cumsum(np.exp(pa.betabin_logpmf(np.arange(L), n, a, b)))
    probs = pa._bbn_probs(n, a, b, L)
    cdf = pa._choice_cdf(probs, n_samples * iterations)
    st = np.random.get_state()
    words, _ = _native.legacy_uniform_words(np.array(st[1], dtype=np.uint32), st[2], 2 * n_samples * iterations)
    return model_cdf, probs, cdf, words


def test_bbn_ks_sim_dev_reproduces_the_recorded_reference_calls(gpu_ctx):
    calls = host.recorded_ks_calls()
    limits = {int(c['sim_limit']) for c in calls}
    assert 4096 in limits and 4097 in limits                                       # histogram in LDS / in the workspace
    for c in calls:
        n_samples, iterations, L = int(np.sum(c['y_values'])), int(c['iterations']), int(c['sim_limit'])
        host.set_state(c['key_before'], c['pos_before'])
        model_cdf, probs, cdf, words = bbn_inputs(int(c['n']), c['a'], c['b'], L, n_samples, iterations)
        for kind in chk.STREAMS:
            ks, = chk.same_bytes([run_bbn(gpu_ctx, kind, f, words, cdf, model_cdf, n_samples, iterations) for f in chk.FILLS])
            np.testing.assert_array_equal(ks, c['ks_sim'])


@pytest.mark.parametrize('sim_limit,n_samples,iterations', [(40, 1, 300), (4096, 517, 3), (4097, 517, 3), (4097, 1, 1),
                                                             (9000, 3, 2500), (5000, 700, 1030)])
@pytest.mark.parametrize('kind', chk.STREAMS)
def test_bbn_ks_sim_dev_against_the_restated_loop(sim_limit, n_samples, iterations, kind, gpu_ctx):
    """numpy's own choice() and a histogram per iteration (test_betabinom_host.numpy_ks_sim). More than 1024 iterations
    above the LDS limit: a workgroup uses its histogram in the workspace again for its next iteration."""
    n, a, b = (60, 0.4, 30.0) if sim_limit == 40 else (20000, 3.0, 20.0)
    np.random.seed(sim_limit + n_samples + iterations)
    model_cdf, probs, cdf, words = bbn_inputs(n, a, b, sim_limit, n_samples, iterations)
    want = host.numpy_ks_sim(model_cdf, probs, n_samples, iterations)
    ks, = chk.same_bytes([run_bbn(gpu_ctx, kind, f, words, cdf, model_cdf, n_samples, iterations) for f in chk.FILLS])
    np.testing.assert_array_equal(ks, want)


def test_bbn_ks_sim_dev_no_iterations_refusal_and_no_allocation(gpu_ctx):
    L, n_samples, iterations = 5000, 100, 7
    np.random.seed(1)
    model_cdf, probs, cdf, words = bbn_inputs(20000, 3.0, 20.0, L, n_samples, iterations)
    want = host.numpy_ks_sim(model_cdf, probs, n_samples, iterations)
    nws = int(_native.lib().pgx_bbn_workspace_bytes(L, iterations))
    assert nws == iterations * L * 4
    d_w, d_cdf, d_model = chk.upload(words), chk.upload(cdf), chk.upload(model_cdf)
    ks, ws = chk.guarded(iterations * 8, 0xFF), chk.guarded(nws, 0xFF)
    gpu_ctx.bbn_ks_sim_dev(d_w.ptr, d_cdf.ptr, d_model.ptr, L, n_samples, 0, ks.ptr, ws.ptr, nws, 0)    # a no-op
    with pytest.raises(_native.PgxError, match='workspace smaller'):
        gpu_ctx.bbn_ks_sim_dev(d_w.ptr, d_cdf.ptr, d_model.ptr, L, n_samples, iterations, ks.ptr, ws.ptr, nws - 1, 0)
    torch.cuda.synchronize()
    assert ks.is_still_garbage() and ws.is_still_garbage()
    chk.assert_no_allocation(lambda: gpu_ctx.bbn_ks_sim_dev(d_w.ptr, d_cdf.ptr, d_model.ptr, L, n_samples, iterations,
                                                            ks.ptr, ws.ptr, nws, 0))
    np.testing.assert_array_equal(ks.numpy(np.float64), want)
    ks.assert_guards_intact(), ws.assert_guards_intact()


# ---- pgx_cluster_greedy_dev -------------------------------------------------------------------------------------------
def cluster_sets():
    rng = np.random.default_rng(11)
    s = rand_seq(rng, 300)
    a, b = rand_nt(rng, 400), rand_nt(rng, 1500)
    windows = params()
    windows.batch_size = 64
    many = test_gpu_cluster._random_families(np.random.default_rng(5), AA_LETTERS, 40, 12, 40, 400)
    assert len(many) > 2 * 64
    return {
        'tiny': (synth.protein_set('tiny').nr_arrays()[:2], params(), False),
        'indels': (pack([s, s[:100] + s[103:], s[:50] + 'WWW' + s[50:], s[5:], s[:-7]]), params(), False),
        'ragged': (pack([rand_seq(rng, n) for n in (11, 12, 500, 40, 41, 2000, 11)]), params(), False),
        'both strands': (pack([a, revcomp(a[:380]), b, revcomp(b)[3:], b[:1400], revcomp(a)[5:250]]), nt_params(), True),
        'three windows': (pack(many), windows, False),
    }


@pytest.mark.parametrize('name', ['tiny', 'indels', 'ragged', 'both strands', 'three windows'])
@pytest.mark.parametrize('want_stats', [True, False])
def test_cluster_greedy_dev_matches_the_oracle(name, want_stats, gpu_ctx):
    (res, off), p, nucleotide = cluster_sets()[name]
    res, off = np.ascontiguousarray(res, dtype=np.uint8), np.ascontiguousarray(off, dtype=np.uint64)
    want = oracle.cluster_greedy(res, off, p)
    for kind in chk.STREAMS:
        with chk.stream_scope(kind) as st:
            d_res, d_off = chk.upload(res), chk.upload(off)
            with chk.unchanged(d_res, d_off):
                got = gpu_ctx.cluster_greedy_dev(d_res.ptr, d_off.ptr, off.size - 1, int(off[-1]), p, stream=st,
                                                 want_stats=want_stats)
        if want_stats:
            (test_gpu_cluster.assert_same_nt if nucleotide else test_gpu_cluster.assert_same)(got, want)
            if name == 'three windows':
                assert got[5]['sweeps'] >= 3
        else:
            assert got[5] is None and got[4] == want[4]
            for i in range(4 if nucleotide else 3):
                np.testing.assert_array_equal(got[i], want[i])


# ---- the whole chain on one side stream ---------------------------------------------------------------------------------
def test_one_chain_on_a_side_stream_without_a_host_synchronisation(gpu_ctx):
    """coordinates -> bitmap -> row counts and pan/core curves -> Heaps fits, and the Bernoulli likelihood of the same
    bitmap: five entries enqueued back to back on one side stream behind a busy kernel, every intermediate buffer full of
    garbage, one synchronisation at the end. An entry that put a launch or a memset on another stream would work on
    buffers that are not written yet."""
    rng = np.random.default_rng(77)
    G, S, n_iter = 3000, 70, 5
    p_true, q_true = rng.uniform(0.3, 0.95, G), rng.uniform(0.9, 0.99, S)
    X = rng.random((G, S)) < np.outer(p_true, q_true)
    row, col = (v.astype(np.int32) for v in np.nonzero(X))
    order = rng.permutation(row.size)
    row, col = row[order], col[order]
    perms = np.array([rng.permutation(S) for _ in range(n_iter)], dtype=np.int32)
    pq = np.concatenate((np.clip(X.mean(axis=1), 0.05, 0.97), np.full(S, 0.98)))
    stride = stride_words(G)
    nws_pc, nws_bn = pan_ws_bytes(G, S, n_iter), bern_ws_bytes(G, S)

    def run(fill):
        with chk.stream_scope('side') as st:
            bits, cnt, counts = chk.guarded(S * stride * 8, fill), chk.guarded(16, fill), chk.guarded(G * 4, fill)
            pan, core, ws_pc = chk.guarded(n_iter * S * 4, fill), chk.guarded(n_iter * S * 4, fill), chk.guarded(nws_pc, fill)
            alpha, kappa = chk.guarded(n_iter * 8, fill), chk.guarded(n_iter * 8, fill)
            out, ws_bn = chk.guarded((1 + G + S) * 8, fill), chk.guarded(nws_bn, fill)
            d_r, d_c, d_perms, d_pq = chk.upload(row), chk.upload(col), chk.upload(perms), chk.upload(pq)
            with chk.unchanged(d_r, d_c, d_perms, d_pq):
                gpu_ctx.presence_bitmap_dev(d_r.ptr, d_c.ptr, row.size, G, S, bits.ptr, st, cnt.ptr)
                gpu_ctx.row_counts_dev(bits.ptr, G, S, counts.ptr, st)
                gpu_ctx.pan_core_dev(bits.ptr, G, S, d_perms.ptr, n_iter, pan.ptr, core.ptr, ws_pc.ptr, nws_pc, st)
                gpu_ctx.heaps_fit_dev(pan.ptr, n_iter, S, alpha.ptr, kappa.ptr, st)
                gpu_ctx.bernoulli_eval_dev(bits.ptr, G, S, d_pq.ptr, out.ptr, ws_bn.ptr, nws_bn, 0, st)
        for b in (bits, cnt, counts, pan, core, ws_pc, alpha, kappa, out, ws_bn):
            b.assert_guards_intact()
        return (bits.numpy(np.uint64).reshape(S, stride), cnt.numpy(np.uint64), counts.numpy(np.int32),
                pan.numpy(np.int32).reshape(n_iter, S), core.numpy(np.int32).reshape(n_iter, S),
                alpha.numpy(np.float64), kappa.numpy(np.float64), out.numpy(np.float64))

    bits, cnt, counts, pan, core, alpha, kappa, out = chk.same_bytes([run(f) for f in chk.FILLS])
    assert np.array_equal(bits, bitmap_reference(row, col, S, stride)) and cnt.tolist() == [0, 0]
    assert np.array_equal(counts, X.sum(axis=1))
    opan, ocore = oracle.pan_core(row, col, None, G, S, perms)
    assert np.array_equal(pan, opan) and np.array_equal(core, ocore)
    oa, ok = heaps_ref.fit_rows(opan)
    np.testing.assert_allclose(alpha, oa, rtol=1e-5)
    np.testing.assert_allclose(kappa, ok, rtol=1e-5)
    ha, hk = gpu_ctx.heaps_fit(opan.astype(np.float64))
    assert alpha.tobytes() == ha.tobytes() and kappa.tobytes() == hk.tobytes()
    # the model's definition in numpy (pgx.h), with the tolerances of test_gpu_bernoulli.assert_evaluation
    P, Q = pq[:G], pq[G:]
    r = np.outer(P, Q)
    t = 1.0 - r
    Xf = X.astype(np.float64)
    ll = float((Xf * np.log(r)).sum() + ((1.0 - Xf) * np.log(t)).sum())
    row_terms, col_terms = ((1.0 - Xf) * Q[None, :] / t).sum(axis=1), ((1.0 - Xf) * P[:, None] / t).sum(axis=0)
    grad = np.concatenate((Xf.sum(axis=1) / P - row_terms, Xf.sum(axis=0) / Q - col_terms))
    scale = np.concatenate((Xf.sum(axis=1) / P + row_terms, Xf.sum(axis=0) / Q + col_terms))
    test_gpu_bernoulli.assert_evaluation(out, ll, grad, scale)
    assert gpu_ctx.bernoulli_load(row, col, G, S) == 0
    assert out.tobytes() == gpu_ctx.bernoulli_eval(pq).tobytes()
