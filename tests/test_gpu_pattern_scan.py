"""The variable-length exact pattern scan on the device (csrc/pattern.hip; include/pgx.h "Exact search for variable-length
patterns") against the bytes.find model (tests/pattern_scan_model.py). Positions and counts: every comparison is
exact. Everything runs twice, the second time with PGX_PATTERN_NARROW_HASH: 3 bits of hash, every position is verified against
every pattern, same output; those runs are capped at two tiles of text (and what a pattern needs beyond them) and 200 patterns."""
import numpy as np
import pytest

import dev_entry_checks as dev
import pattern_scan_model as model
from pangenomix_amd import _native

pytestmark = pytest.mark.gpu

NARROW = 1                                   # PGX_PATTERN_NARROW_HASH
FLAGS = (0, NARROW)
NARROW_MAX_PATTERNS = 200
NONE = model.NONE
ALPHABETS = (None, b'ACGT')
SEEDS = (1, 2, 8, 31, 32, 33, 64)


def tile():
    return int(_native.lib().pgx_pattern_scan_tile())


def check(ctx, text, patterns, seed, flags, lead=0):
    """pattern_load + pattern_query against the model; returns (first, count)"""
    assert not (flags & NARROW) or len(patterns) <= NARROW_MAX_PATTERNS
    want_first, want_count = model.first_count(text, patterns)
    assert ctx.pattern_load(*model.blob(patterns, lead), seed=seed, flags=flags) == len(patterns)
    first, count = ctx.pattern_query(text)
    assert first.dtype == np.uint32 and count.dtype == np.uint32
    assert np.array_equal(first, want_first), 'first differs at %r' % np.flatnonzero(first != want_first)[:10].tolist()
    assert np.array_equal(count, want_count), 'count differs at %r' % np.flatnonzero(count != want_count)[:10].tolist()
    return first, count


@pytest.mark.parametrize('flags', FLAGS)
@pytest.mark.parametrize('alphabet', ALPHABETS, ids=('bytes', 'acgt'))
@pytest.mark.parametrize('seed', SEEDS)
def test_text_sizes(seed, alphabet, flags, gpu_ctx):
    T, S = tile(), seed
    assert T >= 256 and T % 256 == 0
    sizes = sorted({0, 1, S - 1, S, S + 1, T - 1, T, T + 1, 2 * T + S - 2, 3 * T + 5})
    if flags & NARROW:
        sizes = [n for n in sizes if n <= 2 * T + S - 2]                         # (two tiles of positions)
    rng = np.random.default_rng(1000 * S + (alphabet is not None))
    found_any = False
    for n in sizes:
        text, patterns = model.kernel_case(rng, n, S, alphabet, lengths=(S, S + 1, 70, 200))
        first, count = check(gpu_ctx, text, patterns, S, flags)
        if n < S:
            assert (first == NONE).all() and not count.any()
        found_any |= bool(count.any())
        assert first[len(patterns) - 5] == NONE                                  # the one longer than the text
    assert found_any


@pytest.mark.parametrize('flags', FLAGS)
def test_pattern_lengths(flags, gpu_ctx):
    """every length around the 16-byte chunks and the 1 KiB a wave compares per step, cut at odd places; T + 100 bytes that
    start in one tile and end two tiles on"""
    T, S = tile(), 8
    rng = np.random.default_rng(7)
    text = model.random_text(rng, 2 * T + 200)
    patterns, where = [], []
    for i, length in enumerate((S, S + 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 1000, 1023, 1024, 1025, 1041)):
        at = 37 * i + 3
        patterns += [text[at:at + length], text[at:at + length - 1] + bytes([text[at + length - 1] ^ 0x80])]
        where += [at, NONE]
        if length > S + 1:                                                       # differs right behind the seed; in the middle
            for j in (S, length // 2):
                patterns.append(text[at:at + j] + bytes([text[at + j] ^ 0x01]) + text[at + j + 1:at + length])
                where.append(NONE)
    long_at = T - 60
    patterns += [text[long_at:long_at + T + 100], text[long_at:long_at + T + 99] + bytes([text[long_at + T + 99] ^ 0x01])]
    where += [long_at, NONE]
    patterns += [text[len(text) - 300:], text[len(text) - S:] + b'zz', text + b'q']     # ends at text_bytes; past it; too long
    where += [len(text) - 300, NONE, NONE]
    first, count = check(gpu_ctx, text, patterns, S, flags)
    assert first.tolist() == where and count.tolist() == [int(w != NONE) for w in where]


@pytest.mark.parametrize('flags', FLAGS)
@pytest.mark.parametrize('where', ('last', 'byte33', 'middle'))
def test_same_seed_chain(where, flags, gpu_ctx):
    """300 patterns of 450 bytes with the same first 32 bytes (a byte holds 256 values: the place that differs is two bytes
    wide). Exactly the ones planted in the text are found."""
    n = NARROW_MAX_PATTERNS if flags & NARROW else 300
    T, S, L = tile(), 32, 450
    rng = np.random.default_rng(11)
    base = bytearray(model.random_text(rng, L, b'ACGT'))
    at = {'last': L - 2, 'byte33': 32, 'middle': L // 2}[where]
    patterns = []
    for i in range(n):
        p = bytearray(base)
        p[at], p[at + 1] = b'ACGTNRYKMSWBDHV0'[i % 16], b'ACGTNRYKMSWBDHV0123456789'[i // 16]
        patterns.append(bytes(p))
    assert len(set(patterns)) == n
    planted = {3: [100], 64: [700, T + 300], n - 1: [T - 200], 150: [2000, 2600, 3200]}      # pattern -> positions (T - 200: across tiles)
    text = bytearray(model.random_text(rng, T + 800, b'ACGT'))
    for k, places in planted.items():
        for p in places:
            text[p:p + L] = patterns[k]
    first, count = check(gpu_ctx, bytes(text), patterns, S, flags)
    for k in range(n):
        assert (first[k], count[k]) == ((min(planted[k]), len(planted[k])) if k in planted else (NONE, 0)), k


@pytest.mark.parametrize('flags', FLAGS)
def test_prefixes_duplicates_and_overlaps(flags, gpu_ctx):
    T, S = tile(), 8
    rng = np.random.default_rng(13)
    text = bytearray(model.random_text(rng, T + 300))
    word = model.random_text(rng, 90)
    for p in (50, 1000, T - 20):
        text[p:p + 90] = word
    text[2000:2040] = word[:40]                                                  # the prefix alone, once more
    text = bytes(text)
    patterns = [word, word[:40], word, word[:89] + bytes([word[89] ^ 1]), word[:S], word[:40]]
    first, count = check(gpu_ctx, text, patterns, S, flags)
    assert first.tolist() == [50, 50, 50, NONE, 50, 50] and count.tolist() == [3, 4, 3, 0, 4, 4]
    # one repeated byte: every position is an occurrence, overlapping ones included
    for n, L in ((T + 77, 100), (500, 500), (2 * T, S), (300, 299)):
        first, count = check(gpu_ctx, b'\x07' * n, [b'\x07' * L, b'\x07' * (L - 1) + b'\x08'], S, flags)
        assert first.tolist() == [0, NONE] and count.tolist() == [n - L + 1, 0]
    # period 2: every second position
    first, count = check(gpu_ctx, b'AB' * 1000, [b'AB' * 10, b'BA' * 10, b'AB' * 1000, b'BA' * 1000], S, flags)
    assert first.tolist() == [0, 1, 0, NONE] and count.tolist() == [991, 990, 1, 0]


@pytest.mark.parametrize('flags', FLAGS)
def test_hits_on_the_first_and_last_lane_and_in_a_partly_empty_round(flags, gpu_ctx):
    """The last tile has 2 * 256 + 70 positions: in its last round one wave is full, the next holds 6 positions and 58 lanes
    without one, two waves hold none -- and all of them vote. True hits sit on lane 0 and lane 63 of a wave in a full round and
    in that last round, and on the text's very last position."""
    T, S = tile(), 8
    rng = np.random.default_rng(17)
    n_pos = T + 2 * 256 + 70
    text = model.random_text(rng, n_pos + S - 1)
    places = [0, 63, 64, 127, 255, 256 + 63, T, T + 63, T + 192, T + 255, T + 512, T + 512 + 63, T + 512 + 64, n_pos - 1]
    patterns = [text[p:p + min(40, len(text) - p)] for p in places]
    patterns += [text[n_pos - 1:] + b'\x00', model.random_text(rng, 20)]
    first, count = check(gpu_ctx, text, patterns, S, flags)
    assert first.tolist() == places + [NONE, NONE] and count.tolist() == [1] * len(places) + [0, 0]
    # and with no hit anywhere but there
    first, count = check(gpu_ctx, text, [text[n_pos - 1:]], S, flags)
    assert first.tolist() == [n_pos - 1] and count.tolist() == [1]


@pytest.mark.parametrize('flags', FLAGS)
@pytest.mark.parametrize('n_patterns', (0, 1, 2, 63, 64, 65, 1000, 20000))
def test_pattern_counts(n_patterns, flags, gpu_ctx):
    """about half the patterns are cut from the text; some are given twice"""
    if flags & NARROW and n_patterns > NARROW_MAX_PATTERNS:
        n_patterns = NARROW_MAX_PATTERNS
    T, S = tile(), 12
    rng = np.random.default_rng(n_patterns)
    text = model.random_text(rng, 2 * T)
    patterns = []
    for i in range(n_patterns):
        length = int(rng.integers(S, 90))
        if rng.random() < 0.5:
            at = int(rng.integers(0, len(text) - length))
            patterns.append(text[at:at + length])
        else:
            patterns.append(model.random_text(rng, length))
    for i in range(5, n_patterns, 50):
        patterns[i] = patterns[i // 2]
    first, count = check(gpu_ctx, text, patterns, S, flags)
    assert first.shape == (n_patterns,)
    if n_patterns >= 63:
        assert 0 < (count == 0).sum() < n_patterns


def test_load_and_query(gpu_ctx):
    rng = np.random.default_rng(19)
    text1, text2 = model.random_text(rng, 9000, b'ACGT'), model.random_text(rng, 5000, b'ACGT')
    set1 = [text1[i:i + 50 + i % 30] for i in range(0, 8000, 97)] + [text2[100:180]]
    set2 = [text2[i:i + 33] for i in range(0, 4000, 211)] + [text1[:40]]
    gpu_ctx.pattern_load(*model.blob(set1), seed=32)
    a = gpu_ctx.pattern_query(text1)
    b = gpu_ctx.pattern_query(text1)                                             # twice on one load: the same bytes
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    for text in (text1, text2, b'', text1[:31]):
        got, want = gpu_ctx.pattern_query(text), model.first_count(text, set1)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    gpu_ctx.pattern_load(*model.blob(set2), seed=20)                             # a second load replaces the first
    for text in (text1, text2):
        got, want = gpu_ctx.pattern_query(text), model.first_count(text, set2)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    gpu_ctx.pattern_load(*model.blob([]), seed=5)
    assert [x.shape for x in gpu_ctx.pattern_query(text1)] == [(0,), (0,)]


def test_invalid_calls_are_refused_before_anything_is_written():
    """on a context of its own: nothing is loaded yet"""
    lib = _native.lib()
    ctx = _native.Context(0)
    try:
        patterns, off = model.blob([b'ACGTAC', b'GTGTGT', b'AAAA'])
        text = np.frombuffer(b'ACGTACGTGTGTAAAA', dtype=np.uint8)
        out = np.full(6, 0x6E6E6E6E, dtype=np.uint32)
        P = _native._ptr

        def refused(rc, who):
            assert rc == -1, who                                                 # PGX_ERR_INVALID
            assert (out == 0x6E6E6E6E).all(), who
        refused(lib.pgx_pattern_query(ctx._h, P(text), text.size, P(out[:3]), P(out[3:])), 'query before any load')
        assert 'loaded' in lib.pgx_last_error().decode()
        refused(lib.pgx_pattern_load(ctx._h, P(patterns), P(off), 1 << 24, 4, 0), 'n_patterns')
        refused(lib.pgx_pattern_load(ctx._h, P(patterns), P(off), 3, 4, 2), 'flags')
        refused(lib.pgx_pattern_load(ctx._h, P(patterns), P(off), 3, 0, 0), 'seed 0')
        refused(lib.pgx_pattern_load(ctx._h, P(patterns), P(off), 3, 65, 0), 'seed 65')
        refused(lib.pgx_pattern_load(ctx._h, P(patterns), P(off), 3, 5, 0), 'a pattern shorter than the seed')
        down = off.copy()
        down[2] = 1
        refused(lib.pgx_pattern_load(ctx._h, P(patterns), P(down), 3, 1, 0), 'decreasing offsets')
        big = off.copy()
        big[3] = 1 << 32
        refused(lib.pgx_pattern_load(ctx._h, P(patterns), P(big), 3, 4, 0), 'blob of 2^32 bytes')
        refused(lib.pgx_pattern_query(ctx._h, P(text), text.size, P(out[:3]), P(out[3:])), 'a refused load loads nothing')
        assert lib.pgx_pattern_workspace_bytes(1 << 32, 3) == 0 and lib.pgx_pattern_workspace_bytes(5, 1 << 24) == 0
        assert lib.pgx_pattern_workspace_bytes(16, 3) == 64 * 8 + 32768 and lib.pgx_pattern_workspace_bytes(0, 0) > 0
        ctx.pattern_load(patterns, off, seed=4)
        refused(lib.pgx_pattern_query(ctx._h, P(text), 1 << 32, P(out[:3]), P(out[3:])), 'text_bytes')
        refused(lib.pgx_pattern_load(ctx._h, P(patterns), P(off), 3, 5, 0), 'a refused load ...')
        first, count = ctx.pattern_query(text)                                   # ... leaves the loaded set in place
        assert first.tolist() == [0, 6, 12] and count.tolist() == [1, 1, 1]
        with pytest.raises(ValueError):
            ctx.pattern_load(patterns, off + np.uint64(1), seed=4)
        # the device entry refuses the same without touching its buffers
        g = dev.guarded(4096, 0x5A)
        ws_bytes = lib.pgx_pattern_workspace_bytes(16, 3)
        for n, seed, flags, text_bytes, ws, ws_at in ((1 << 24, 4, 0, 16, 1 << 30, 0), (3, 4, 2, 16, ws_bytes, 0),
                                                      (3, 0, 0, 16, ws_bytes, 0), (3, 65, 0, 16, ws_bytes, 0),
                                                      (3, 4, 0, 1 << 32, ws_bytes, 0), (3, 4, 0, 16, ws_bytes - 8, 0),
                                                      (3, 4, 0, 16, 0, 0), (3, 4, 0, 16, ws_bytes, 8)):
            with pytest.raises(_native.PgxError) as e:
                ctx.pattern_scan_dev(g.ptr, text_bytes, g.ptr, g.ptr, n, seed, g.ptr, g.ptr, g.ptr + ws_at, ws, flags)
            assert e.value.status == -1
        assert g.is_still_garbage()
        g.assert_guards_intact()
    finally:
        ctx.close()


# -- the device entry ------------------------------------------------------------------------------------------------------
def dev_case(seed_bytes, rng_seed, n_text):
    """a text whose last bytes are the seed of a pattern that goes on with the guard band's byte: read past text_bytes, it
    would match"""
    rng = np.random.default_rng(rng_seed)
    text, patterns = model.kernel_case(rng, n_text, seed_bytes, None, lengths=(seed_bytes, 17, 64, 129, 1000, 1500))
    patterns.append(text[n_text - seed_bytes:] + bytes([dev.GUARD_BYTE]) * 24)
    patterns.append(text[n_text - 100:] + bytes([dev.GUARD_BYTE]))
    patterns.append(text[5:305])
    return text, patterns


def run_dev(ctx, text, patterns, seed, flags, fill, stream, shift=0, lead=0):
    pb, po = model.blob(patterns, lead)
    data = np.frombuffer(text, dtype=np.uint8)
    n = len(patterns)
    ws_bytes = _native.lib().pgx_pattern_workspace_bytes(pb.size, n)
    assert ws_bytes > 0
    with dev.stream_scope(stream) as handle:
        # the text sits at the very end of its allocation's payload, `shift` bytes off 16-byte alignment, a guard band behind it
        d_text = dev.guarded(shift + data.size, 0x5A)
        if data.size:
            d_text.raw[dev.GUARD + shift:dev.GUARD + shift + data.size] = dev.upload(data).dev
        d_pb, d_po = dev.upload(pb), dev.upload(po)
        first, count, ws = dev.guarded(4 * n, fill), dev.guarded(4 * n, fill), dev.guarded(ws_bytes, fill)
        with dev.unchanged(d_text.raw, d_pb, d_po):
            ctx.pattern_scan_dev(d_text.ptr + shift, data.size, d_pb.ptr, d_po.ptr, n, seed, first.ptr, count.ptr, ws.ptr,
                                 ws_bytes, flags, handle)
    for buf in (first, count, ws):
        buf.assert_guards_intact()
    return first.numpy(np.uint32), count.numpy(np.uint32)


@pytest.mark.parametrize('flags', FLAGS)
@pytest.mark.parametrize('stream', dev.STREAMS)
def test_device_entry_on_caller_tensors(stream, flags, gpu_ctx):
    T = tile()
    for seed, n_text, shift in ((8, 2 * T + 100, 0), (32, T + 1, 1), (1, 600, 4), (64, T + 63, 15)):
        text, patterns = dev_case(seed, seed + shift, n_text)
        want = model.first_count(text, patterns)
        assert want[1][-3] == 0 and want[1][-2] == 0 and want[1][-1] == 1
        per_fill = []
        for fill in dev.FILLS:                                        # outputs and the workspace pre-filled with garbage
            got = run_dev(gpu_ctx, text, patterns, seed, flags, fill, stream, shift=shift, lead=shift % 3)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            per_fill.append(got)
        dev.same_bytes(per_fill)
    # a text shorter than the seed, and an empty one: first and count are still written
    for text in (b'abc', b''):
        first, count = run_dev(gpu_ctx, text, [b'abcdefgh', b'abcdefghi'], 8, flags, 0x5A, stream)
        assert first.tolist() == [NONE, NONE] and count.tolist() == [0, 0]


def test_device_entry_does_not_allocate(gpu_ctx):
    text, patterns = dev_case(16, 23, 3 * tile() + 5)
    pb, po = model.blob(patterns)
    n = len(patterns)
    ws_bytes = _native.lib().pgx_pattern_workspace_bytes(pb.size, n)
    d_text, d_pb, d_po = dev.upload(np.frombuffer(text, dtype=np.uint8)), dev.upload(pb), dev.upload(po)
    first, count, ws = dev.guarded(4 * n, 0xFF), dev.guarded(4 * n, 0xFF), dev.guarded(ws_bytes, 0xFF)
    dev.assert_no_allocation(lambda: gpu_ctx.pattern_scan_dev(d_text.ptr, len(text), d_pb.ptr, d_po.ptr, n, 16, first.ptr,
                                                              count.ptr, ws.ptr, ws_bytes))
    want = model.first_count(text, patterns)
    assert np.array_equal(first.numpy(np.uint32), want[0]) and np.array_equal(count.numpy(np.uint32), want[1])
    gpu_ctx.pattern_scan_dev(None, 0, None, None, 0, 16, None, None, None, 0)    # n_patterns = 0 does nothing
