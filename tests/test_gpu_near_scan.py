"""The bounded-mismatch pattern scan on the device (csrc/near.hip; include/pgx.h "Bounded-mismatch search for variable-length
patterns") against the brute-force model (tests/near_scan_model.py: every pattern against every window, no blocks,
no hashes). Everything runs twice, the second time with PGX_NEAR_NARROW_HASH: 3 bits of hash, every position is verified against
every indexed block, same output; those runs are capped at two tiles of text and 200 patterns."""
import numpy as np
import pytest

import dev_entry_checks as dev
import near_scan_model as model
from pattern_scan_model import blob, random_text
from pangenomix_amd import _native

pytestmark = pytest.mark.gpu

NARROW = 1                                   # PGX_NEAR_NARROW_HASH
FLAGS = (0, NARROW)
NARROW_MAX_PATTERNS = 200
NONE = model.NONE
NO_SEP = model.NO_SEPARATOR
BLOCKS = (1, 8, 13, 19, 32, 64)


def tile():
    return int(_native.lib().pgx_near_scan_tile())


def check(ctx, text, patterns, mm, block, flags, separator=NO_SEP, active=None, lead=0):
    """near_load + near_query against the model; returns best"""
    assert len(text) <= 2 * tile() + block or not (flags & NARROW)
    assert not (flags & NARROW) or len(patterns) <= NARROW_MAX_PATTERNS
    want = model.best(text, patterns, mm, separator, active)
    assert ctx.near_load(*blob(patterns, lead), max_mismatch=mm, block=block, flags=flags) == len(patterns)
    got = ctx.near_query(text, separator=separator, active=active)
    assert got.dtype == np.uint64 and got.shape == (len(patterns),)
    assert np.array_equal(got, want), 'best differs at %r' % np.flatnonzero(got != want)[:10].tolist()
    return got


def spread(rng, length, n):
    """n distinct places in a string of `length` bytes"""
    return sorted(rng.choice(length, size=n, replace=False).tolist())


def one_per_block(block, blocks, length):
    """one place inside each of the indexed blocks `blocks`"""
    return [j * block + (5 * j + 3) % block for j in blocks]


@pytest.mark.parametrize('flags', FLAGS)
@pytest.mark.parametrize('block', BLOCKS)
def test_text_sizes(block, flags, gpu_ctx):
    T, B = tile(), block
    assert T >= 256 and T % 256 == 0
    sizes = sorted({0, B - 1, B, B + 1, T - 1, T, T + 1, 2 * T + B - 2})
    rng = np.random.default_rng(100 + B)
    found = missed = 0
    for n in sizes:
        text = random_text(rng, n)
        patterns, mm = [], []
        for length in (B, B + 1, 3 * B, 70, 200):
            m = min(2, length // B - 1)
            if B <= length <= n and m >= 0:
                for at in (int(rng.integers(0, n - length + 1)), n - length):         # anywhere; ending exactly at text_bytes
                    window = text[at:at + length]
                    patterns += [model.mutate(window, spread(rng, length, m)), model.mutate(window, spread(rng, length, m + 1))]
                    mm += [m, m]
        patterns += [text + random_text(rng, B), random_text(rng, B + 7), random_text(rng, 3 * B)]
        mm += [0, 0, 2]
        best = check(gpu_ctx, text, patterns, mm, B, flags)
        if n < B:
            assert (best == NONE).all()
        found += int((best != NONE).sum())
        missed += int((best == NONE).sum())
        assert best[len(patterns) - 3] == NONE                                   # the one longer than the text
    assert found > 10 and missed > 10


@pytest.mark.parametrize('flags', FLAGS)
@pytest.mark.parametrize('m,block,length', ((0, 13, 50), (1, 13, 50), (2, 13, 50), (22, 19, 450), (255, 4, 1100), (255, 1, 700)))
def test_distance_exactly_m_is_found_and_m_plus_one_is_not(m, block, length, flags, gpu_ctx):
    """one mismatch in each of the first m indexed blocks: only the last indexed block leads to the window; a further mismatch
    in that block and the window is out of reach and beyond the bound"""
    rng = np.random.default_rng(m)
    T = tile()
    p_in, p_out, p_any = (random_text(rng, length, b'ACGT') for _ in range(3))
    text = bytearray(random_text(rng, T + 2 * length + 300, b'ACGT'))
    text[100:100 + length] = model.mutate(p_in, one_per_block(block, range(m), length))
    text[T - 50:T - 50 + length] = model.mutate(p_out, one_per_block(block, range(m + 1), length))
    text[T + length:T + 2 * length] = model.mutate(p_any, spread(rng, length, m))
    best = check(gpu_ctx, bytes(text), [p_in, p_out, p_any], [m, m, m], block, flags)
    assert best.tolist() == [(m << 32) | 100, NONE, (m << 32) | (T + length)]


@pytest.mark.parametrize('flags', FLAGS)
def test_every_block_index_leads_to_the_window(flags, gpu_ctx):
    """450 bytes, m = 22, blocks of 19: for every j a window in which only block j is intact, each other indexed block holding
    one mismatch -- block 22's seed sits 418 bytes behind the window's start. In two texts of at most two tiles."""
    L, m, B = 450, 22, 19
    rng = np.random.default_rng(23)
    for js in (range(0, 12), range(12, 23)):
        patterns = [random_text(rng, L, b'ACGT') for _ in js]
        text = bytearray(random_text(rng, 60 + len(js) * 520, b'ACGT'))
        assert len(text) <= 2 * tile()
        where = []
        for n, j in enumerate(js):
            at = 31 + n * 520
            text[at:at + L] = model.mutate(patterns[n], one_per_block(B, [b for b in range(m + 1) if b != j], L))
            where.append((m << 32) | at)
        best = check(gpu_ctx, bytes(text), patterns, [m] * len(js), B, flags)
        assert best.tolist() == where


@pytest.mark.parametrize('flags', FLAGS)
def test_windows_that_start_in_one_tile_and_survive_in_the_next(flags, gpu_ctx):
    L, m, B = 450, 22, 19
    T = tile()
    rng = np.random.default_rng(29)
    # (where the window starts, the one block that survives): block 10, 90 bytes into the second tile; block 0, lying across
    # the tiles' joint; block 22, 18 bytes into the second tile; block 22 ending with the first tile's last byte
    for at, alive in ((T - 100, 10), (T - 5, 0), (T - 400, 22), (T - 418 - B, 22)):
        pattern, other = random_text(rng, L, b'ACGT'), random_text(rng, L, b'ACGT')
        text = bytearray(random_text(rng, 2 * T, b'ACGT'))
        text[at:at + L] = model.mutate(pattern, one_per_block(B, [b for b in range(m + 1) if b != alive], L))
        best = check(gpu_ctx, bytes(text), [other, pattern], [m, m], B, flags)
        assert best.tolist() == [NONE, (m << 32) | at]


@pytest.mark.parametrize('flags', FLAGS)
def test_windows_at_the_ends_of_the_text(flags, gpu_ctx):
    """a surviving block so near the text's start that the window would begin before 0; a window that ends exactly at
    text_bytes, and one that would end one byte past it"""
    B, m = 13, 3
    rng = np.random.default_rng(31)
    p = random_text(rng, 60, b'ACGT')
    for j in (1, 2, 3):
        text = p[j * B:] + random_text(rng, 300, b'ACGT')                         # block j at position 0: the window at -j * B
        assert (check(gpu_ctx, text, [p], [m], B, flags) == NONE).all()
        text = p[j * B - 1:] + random_text(rng, 300, b'ACGT')                     # one byte short of fitting
        assert (check(gpu_ctx, text, [p], [m], B, flags) == NONE).all()
    body = random_text(rng, 500, b'ACGT')
    text = body + model.mutate(p, [5, 20])                                       # ends exactly at text_bytes
    past = text[len(text) - 59:] + b'A'                                          # would end one byte past it
    best = check(gpu_ctx, text, [p, past, past[:59]], [m, m, m], B, flags)
    assert best.tolist() == [(2 << 32) | 500, NONE, len(text) - 59]
    best = check(gpu_ctx, p[:59], [p], [m], B, flags)                             # the text is one byte shorter than the pattern
    assert best.tolist() == [NONE]


@pytest.mark.parametrize('flags', FLAGS)
def test_pattern_lengths(flags, gpu_ctx):
    """every length around the 16-byte chunks and the 1 KiB a wave compares per step: the only mismatch in the last byte, and
    mismatches on both sides of the 1 KiB step"""
    T, B = tile(), 8
    rng = np.random.default_rng(37)
    text = random_text(rng, 2 * T)
    patterns, mm, want = [], [], []
    for i, length in enumerate((B, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 1041)):
        at = 41 * i + 3
        window = text[at:at + length]
        last = model.mutate(window, [length - 1])
        patterns += [window, last]
        mm += [0, 0]
        want += [at, NONE]
        if length >= 2 * B:
            patterns += [last, model.mutate(window, [0, length - 1])]
            mm += [1, 1]
            want += [(1 << 32) | at, NONE]
        if length > 1024:
            across = model.mutate(window, [1023, 1024])
            patterns += [across, across, model.mutate(window, [3, 1023, 1024]), model.mutate(window, [3, 1022, 1023, length - 1])]
            mm += [2, 1, 2, 3]
            want += [(2 << 32) | at, NONE, NONE, NONE]
    best = check(gpu_ctx, text, patterns, mm, B, flags)
    assert best.tolist() == want


@pytest.mark.parametrize('flags', FLAGS)
@pytest.mark.parametrize('separator', (0, ord('N')))
def test_separator(separator, flags, gpu_ctx):
    B, m = 13, 1
    rng = np.random.default_rng(41)
    sep = bytes([separator])
    p_clean, p_holds = random_text(rng, 50, b'ACGT'), random_text(rng, 20, b'ACGT') + sep + random_text(rng, 29, b'ACGT')
    p_far = random_text(rng, 1100, b'ACGT')
    text = bytearray(random_text(rng, 3000, b'ACGT'))
    text[100:150] = p_clean[:30] + sep + p_clean[31:]                            # one mismatch, and it is the separator
    text[300:350] = p_holds                                                      # exact, but the window holds the separator
    text[500:1600] = p_far[:1090] + sep + p_far[1091:]                           # the separator in the second 1 KiB step
    text[2000:2050] = model.mutate(p_clean, [7])
    text = bytes(text)
    patterns, mm = [p_clean, p_holds, p_far], [m, m, m]
    best = check(gpu_ctx, text, patterns, mm, B, flags, separator=separator)
    assert best.tolist() == [(1 << 32) | 2000, NONE, NONE]
    best = check(gpu_ctx, text, patterns, mm, B, flags, separator=NO_SEP)
    assert best.tolist() == [(1 << 32) | 100, 300, (1 << 32) | 500]
    best = check(gpu_ctx, text, patterns, mm, B, flags, separator=ord('#'))      # a byte the text does not hold
    assert best.tolist() == [(1 << 32) | 100, 300, (1 << 32) | 500]


@pytest.mark.parametrize('flags', FLAGS)
def test_fewest_mismatches_then_the_smallest_position(flags, gpu_ctx):
    B, m = 13, 2
    rng = np.random.default_rng(43)
    p, q = random_text(rng, 50, b'ACGT'), random_text(rng, 50, b'ACGT')
    text = bytearray(random_text(rng, tile() + 600, b'ACGT'))
    for at, places in ((100, [3, 30]), (1000, [17]), (2000, [40]), (tile() + 200, [0])):
        text[at:at + 50] = model.mutate(p, places)
    for at, places in ((400, [1, 2, 3]), (3000, [20, 21]), (3500, [48, 49])):
        text[at:at + 50] = model.mutate(q, places)
    best = check(gpu_ctx, bytes(text), [p, q], [m, m], B, flags)
    assert best.tolist() == [(1 << 32) | 1000, (2 << 32) | 3000]


@pytest.mark.parametrize('flags', FLAGS)
@pytest.mark.parametrize('budget', ('own', 'all'))
def test_chain_of_patterns_that_share_every_block(budget, flags, gpu_ctx):
    """300 patterns of 450 bytes that differ in their last two bytes only, behind the 23 indexed blocks. 'own': the planted
    patterns have the budget of their window (0, 1, 22), every other one 0 and returns all-ones. 'all': 22 everywhere -- every
    block is a run of equal entries, and every pattern finds the exact window of its neighbour."""
    n = 300 if not flags & NARROW else (NARROW_MAX_PATTERNS if budget == 'own' else 40)
    T, B, L, M = tile(), 19, 450, 22
    rng = np.random.default_rng(47)
    base = bytearray(random_text(rng, L, b'ACGT'))
    patterns = []
    for i in range(n):
        p = bytearray(base)
        p[L - 2], p[L - 1] = b'ACGTNRYKMSWBDHV0'[i % 16], b'ACGTNRYKMSWBDHV0123456789'[i // 16]
        patterns.append(bytes(p))
    assert len(set(patterns)) == n
    planted = {3: (100, 0), n // 3: (T - 200, 1), n - 1: (T + 300, M)}           # pattern -> (position, distance)
    text = bytearray(random_text(rng, T + 800, b'ACGT'))
    for k, (at, d) in planted.items():
        text[at:at + L] = model.mutate(patterns[k], one_per_block(B, range(d), L))
    mm = [M] * n if budget == 'all' else [planted[k][1] if k in planted else 0 for k in range(n)]
    best = check(gpu_ctx, bytes(text), patterns, mm, B, flags)
    if budget == 'own':
        assert best[3] == 100 and best[n // 3] == (1 << 32) | (T - 200)
        assert best[n - 1] >> np.uint64(32) <= 2                                  # (a neighbour's window is nearer than its own)
        assert all(best[k] == NONE for k in range(n) if k not in planted)
    else:
        assert (best != NONE).all() and int(best.max() >> np.uint64(32)) <= 2


@pytest.mark.parametrize('flags', FLAGS)
def test_active(flags, gpu_ctx):
    B = 8
    rng = np.random.default_rng(53)
    text = random_text(rng, tile() + 500, b'ACGT')
    patterns = [model.mutate(text[at:at + 40], [9] if i % 2 else []) for i, at in enumerate(range(10, 3000, 150))]
    patterns.append(random_text(rng, 40, b'ACGT'))
    n = len(patterns)
    mm = [1] * n
    everything = check(gpu_ctx, text, patterns, mm, B, flags)
    assert (everything[:-1] != NONE).all() and everything[-1] == NONE
    some = (np.arange(n) % 3 != 1).astype(np.uint8)
    best = check(gpu_ctx, text, patterns, mm, B, flags, active=some)
    assert (best[some == 0] == NONE).all() and np.array_equal(best[some == 1], everything[some == 1])
    assert (check(gpu_ctx, text, patterns, mm, B, flags, active=np.zeros(n, dtype=np.uint8)) == NONE).all()
    assert np.array_equal(check(gpu_ctx, text, patterns, mm, B, flags, active=np.full(n, 7, dtype=np.uint8)), everything)
    assert np.array_equal(check(gpu_ctx, text, patterns, mm, B, flags, active=None), everything)


@pytest.mark.parametrize('flags', FLAGS)
def test_without_mismatches_the_positions_are_the_exact_scan_s(flags, gpu_ctx):
    B = 12
    rng = np.random.default_rng(59)
    text = random_text(rng, 2 * tile(), b'ACGT')
    patterns = [text[at:at + 30 + at % 50] for at in range(0, 8000, 173)] + [random_text(rng, 33, b'ACGT') for _ in range(9)]
    patterns += [text[500:530], b'A' * 12]
    best = check(gpu_ctx, text, patterns, [0] * len(patterns), B, flags)
    gpu_ctx.pattern_load(*blob(patterns), seed=B, flags=flags)
    first, count = gpu_ctx.pattern_query(text)
    assert ((best >> np.uint64(32) == 0) == (count > 0)).all()
    found = count > 0
    assert np.array_equal((best & np.uint64(0xFFFFFFFF))[found].astype(np.uint32), first[found])
    assert (best[~found] == NONE).all() and found.sum() >= 47


def test_load_and_query(gpu_ctx):
    rng = np.random.default_rng(61)
    text1, text2 = random_text(rng, 9000, b'ACGT'), random_text(rng, 5000, b'ACGT')
    set1 = [model.mutate(text1[i:i + 50 + i % 30], [i % 50]) for i in range(0, 8000, 297)] + [text2[100:180]]
    set2 = [model.mutate(text2[i:i + 33], [i % 33, (i + 9) % 33]) for i in range(0, 4000, 411)] + [text1[:40]]
    mm1, mm2 = [1] * len(set1), [2] * len(set2)
    gpu_ctx.near_load(*blob(set1), max_mismatch=mm1, block=25)
    a = gpu_ctx.near_query(text1)
    b = gpu_ctx.near_query(text1)                                                # twice on one load: the same bytes
    assert a.tobytes() == b.tobytes()
    for text in (text1, text2, b'', text1[:24]):
        assert np.array_equal(gpu_ctx.near_query(text), model.best(text, set1, mm1))
    gpu_ctx.near_load(*blob(set2), max_mismatch=mm2, block=11)                    # a second load replaces the first
    for text in (text1, text2):
        assert np.array_equal(gpu_ctx.near_query(text, separator=0), model.best(text, set2, mm2, 0))
    gpu_ctx.near_load(*blob([]), max_mismatch=[], block=5)
    assert gpu_ctx.near_query(text1).shape == (0,)


@pytest.mark.parametrize('flags', FLAGS)
def test_hits_on_the_first_and_last_lane_and_in_a_partly_empty_round(flags, gpu_ctx):
    """The cases of the pattern scan's test of this name: the last tile has 2 * 256 + 70 positions, so in its last round one
    wave is full, the next holds 6 positions and 58 lanes without one, two waves hold none -- and all of them vote. Windows
    sit on lane 0 and lane 63 of a wave in a full round and in that last round, and on the text's very last position."""
    T, B = tile(), 8
    rng = np.random.default_rng(17)
    n_pos = T + 2 * 256 + 70
    text = random_text(rng, n_pos + B - 1)
    places = [0, 63, 64, 127, 255, 256 + 63, T, T + 63, T + 192, T + 255, T + 512, T + 512 + 63, T + 512 + 64, n_pos - 1]
    patterns = [text[p:p + min(40, len(text) - p)] for p in places]
    mm = [len(p) // B - 1 for p in patterns]
    patterns = [model.mutate(p, [B + 2] if m else []) for p, m in zip(patterns, mm)]                  # block 0 survives
    patterns += [text[n_pos - 1:] + b'\x00', random_text(rng, 20)]
    mm += [0, 1]
    best = check(gpu_ctx, text, patterns, mm, B, flags)
    assert best.tolist() == [(min(m, 1) << 32) | p for p, m in zip(places, mm)] + [NONE, NONE]
    # and with no hit anywhere but there
    assert check(gpu_ctx, text, [text[n_pos - 1:]], [0], B, flags).tolist() == [n_pos - 1]


def test_invalid_calls_are_refused_before_anything_is_written():
    """on a context of its own: nothing is loaded yet"""
    lib = _native.lib()
    ctx = _native.Context(0)
    try:
        patterns, off = blob([b'ACGTAC', b'GTGTGT', b'AAAA'])
        mm = np.array([1, 0, 0], dtype=np.uint8)
        text = np.frombuffer(b'ACGTACGTGTGTAAAA', dtype=np.uint8)
        out = np.full(3, 0x6E6E6E6E6E6E6E6E, dtype=np.uint64)
        P = _native._ptr

        def refused(rc, who):
            assert rc == -1, who                                                 # PGX_ERR_INVALID
            assert (out == 0x6E6E6E6E6E6E6E6E).all(), who
        refused(lib.pgx_near_query(ctx._h, P(text), text.size, NO_SEP, None, P(out)), 'query before any load')
        assert 'loaded' in lib.pgx_last_error().decode()
        refused(lib.pgx_near_load(ctx._h, P(patterns), P(off), 1 << 24, P(mm), 2, 0), 'n_patterns')
        refused(lib.pgx_near_load(ctx._h, P(patterns), P(off), 3, P(mm), 2, 2), 'flags')
        refused(lib.pgx_near_load(ctx._h, P(patterns), P(off), 3, P(mm), 0, 0), 'block 0')
        refused(lib.pgx_near_load(ctx._h, P(patterns), P(off), 3, P(mm), 65, 0), 'block 65')
        refused(lib.pgx_near_load(ctx._h, P(patterns), P(off), 3, P(mm), 4, 0), '(m + 1) * block > L for pattern 0')
        none = np.zeros(3, dtype=np.uint8)
        refused(lib.pgx_near_load(ctx._h, P(patterns), P(off), 3, P(none), 5, 0), 'block > L for pattern 2')
        down = off.copy()
        down[2] = 1
        refused(lib.pgx_near_load(ctx._h, P(patterns), P(down), 3, P(mm), 1, 0), 'decreasing offsets')
        big = off.copy()
        big[3] = 1 << 32
        refused(lib.pgx_near_load(ctx._h, P(patterns), P(big), 3, P(mm), 3, 0), 'blob of 2^32 bytes')
        refused(lib.pgx_near_query(ctx._h, P(text), text.size, NO_SEP, None, P(out)), 'a refused load loads nothing')
        ws = lib.pgx_near_workspace_bytes
        assert ws(1 << 32, 3, 4) == 0 and ws(5, 1 << 24, 4) == 0 and ws(5, 3, 1 << 30) == 0
        assert ws(16, 3, 4) == 64 * 8 + 32768 + 16 and ws(0, 0, 0) > 0 and ws(16, 3, 33) == 128 * 8 + 32768 + 16
        ctx.near_load(patterns, off, mm, block=3)
        refused(lib.pgx_near_query(ctx._h, P(text), 1 << 32, NO_SEP, None, P(out)), 'text_bytes')
        refused(lib.pgx_near_query(ctx._h, P(text), text.size, 0x101, None, P(out)), 'separator')
        refused(lib.pgx_near_load(ctx._h, P(patterns), P(off), 3, P(mm), 4, 0), 'a refused load ...')
        best = ctx.near_query(text)                                              # ... leaves the loaded set in place
        assert best.tolist() == [0, 6, 12]
        with pytest.raises(ValueError):
            ctx.near_load(patterns, off + np.uint64(1), mm, block=3)
        with pytest.raises(ValueError):
            ctx.near_load(patterns, off, mm[:2], block=3)
        # the device entry refuses the same without touching its buffers
        g = dev.guarded(4096, 0x5A)
        ws_bytes = ws(16, 3, 4)
        for n, block, flags, text_bytes, sep, n_blocks, size, ws_at in (
                (1 << 24, 3, 0, 16, 0, 4, 1 << 30, 0), (3, 3, 2, 16, 0, 4, ws_bytes, 0), (3, 0, 0, 16, 0, 4, ws_bytes, 0),
                (3, 65, 0, 16, 0, 4, ws_bytes, 0), (3, 3, 0, 1 << 32, 0, 4, ws_bytes, 0), (3, 3, 0, 16, 0x101, 4, ws_bytes, 0),
                (3, 3, 0, 16, 0, 1 << 30, 1 << 40, 0), (3, 3, 0, 16, 0, 4, ws_bytes - 8, 0), (3, 3, 0, 16, 0, 33, ws_bytes, 0),
                (3, 3, 0, 16, 0, 4, 0, 0), (3, 3, 0, 16, 0, 4, ws_bytes, 8)):
            with pytest.raises(_native.PgxError) as e:
                ctx.near_scan_dev(g.ptr, text_bytes, sep, g.ptr, g.ptr, n, g.ptr, block, n_blocks, None, g.ptr, g.ptr + ws_at,
                                  size, flags)
            assert e.value.status == -1
        assert g.is_still_garbage()
        g.assert_guards_intact()
    finally:
        ctx.close()


# -- the device entry ------------------------------------------------------------------------------------------------------
def dev_case(block, rng_seed, n_text):
    """a text over every byte value and patterns within their budgets, beyond them and absent -- among them one whose
    continuation behind the text's last bytes is the guard band's byte: read past text_bytes, it would be a window"""
    rng = np.random.default_rng(rng_seed)
    text = random_text(rng, n_text)
    patterns, mm = [], []
    for length in (block, 17, 64, 129, 450, 1041, 1500):
        m = min(length // block - 1, 22)
        if m < 0 or length > n_text:
            continue
        for at in (int(rng.integers(0, n_text - length + 1)), n_text - length):
            window = text[at:at + length]
            patterns += [model.mutate(window, spread(rng, length, m)), model.mutate(window, spread(rng, length, m + 1))]
            mm += [m, m]
    m = 256 // block - 1 if block <= 64 else 0
    patterns += [model.mutate(text[7:7 + 256], one_per_block(block, range(min(m, 255)), 256))]
    mm += [min(m, 255)]
    patterns.append(text[n_text - 2 * block:] + bytes([dev.GUARD_BYTE]) * 24)      # two blocks in the text, the tail behind it
    mm.append(1)
    patterns.append(text[n_text - 100:] + bytes([dev.GUARD_BYTE]))
    mm.append(100 // block - 1 if 100 // block - 1 < 5 else 5)
    patterns.append(text[5:305])
    mm.append(0)
    return text, patterns, mm


def run_dev(ctx, text, patterns, mm, block, flags, fill, stream, separator=NO_SEP, active=None, shift=0, lead=0):
    pb, po = blob(patterns, lead)
    data = np.frombuffer(text, dtype=np.uint8)
    n = len(patterns)
    mm = np.asarray(mm, dtype=np.uint8)
    n_blocks = int(mm.astype(np.int64).sum()) + n
    ws_bytes = _native.lib().pgx_near_workspace_bytes(pb.size, n, n_blocks)
    assert ws_bytes > 0
    with dev.stream_scope(stream) as handle:
        # the text sits at the very end of its allocation's payload, `shift` bytes off 16-byte alignment, a guard band behind it
        d_text = dev.guarded(shift + data.size, 0x5A)
        if data.size:
            d_text.raw[dev.GUARD + shift:dev.GUARD + shift + data.size] = dev.upload(data).dev
        d_pb, d_po, d_mm = dev.upload(pb), dev.upload(po), dev.upload(mm)
        d_active = dev.upload(np.asarray(active, dtype=np.uint8)) if active is not None else None
        best, ws = dev.guarded(8 * n, fill), dev.guarded(ws_bytes, fill)
        inputs = [d_text.raw, d_pb, d_po, d_mm] + ([d_active] if d_active is not None else [])
        with dev.unchanged(*inputs):
            ctx.near_scan_dev(d_text.ptr + shift, data.size, separator, d_pb.ptr, d_po.ptr, n, d_mm.ptr, block, n_blocks,
                              d_active.ptr if d_active is not None else None, best.ptr, ws.ptr, ws_bytes, flags, handle)
    for buf in (best, ws):
        buf.assert_guards_intact()
    return (best.numpy(np.uint64),)


@pytest.mark.parametrize('flags', FLAGS)
@pytest.mark.parametrize('stream', dev.STREAMS)
def test_device_entry_on_caller_tensors(stream, flags, gpu_ctx):
    T = tile()
    for block, n_text, shift in ((8, T + 1700, 0), (32, T + 1, 1), (1, 600, 4), (64, T + 63, 15)):
        text, patterns, mm = dev_case(block, block + shift, n_text)
        active = (np.arange(len(patterns)) % 5 != 2).astype(np.uint8) if shift == 1 else None
        if active is not None:
            active[-3:] = 1
        sep = text[50] if shift == 4 else NO_SEP
        want = model.best(text, patterns, mm, sep, active)
        assert want[-3] == NONE and want[-2] == NONE and (want[-1] == 5 or sep != NO_SEP)
        per_fill = []
        for fill in dev.FILLS:                                        # outputs and the workspace pre-filled with garbage
            got = run_dev(gpu_ctx, text, patterns, mm, block, flags, fill, stream, sep, active, shift=shift, lead=shift % 3)
            assert np.array_equal(got[0], want), np.flatnonzero(got[0] != want)[:10].tolist()
            per_fill.append(got)
        dev.same_bytes(per_fill)
    # a text shorter than the block, and an empty one: best is still written
    for text in (b'abc', b''):
        got = run_dev(gpu_ctx, text, [b'abcdefgh', b'abcdefghi'], [0, 0], 8, flags, 0x5A, stream)
        assert got[0].tolist() == [NONE, NONE]


def test_device_entry_does_not_allocate(gpu_ctx):
    text, patterns, mm = dev_case(16, 23, 3 * tile() + 5)
    pb, po = blob(patterns)
    n = len(patterns)
    mm = np.asarray(mm, dtype=np.uint8)
    n_blocks = int(mm.astype(np.int64).sum()) + n
    ws_bytes = _native.lib().pgx_near_workspace_bytes(pb.size, n, n_blocks)
    d_text, d_pb, d_po, d_mm = dev.upload(np.frombuffer(text, dtype=np.uint8)), dev.upload(pb), dev.upload(po), dev.upload(mm)
    best, ws = dev.guarded(8 * n, 0xFF), dev.guarded(ws_bytes, 0xFF)
    dev.assert_no_allocation(lambda: gpu_ctx.near_scan_dev(d_text.ptr, len(text), NO_SEP, d_pb.ptr, d_po.ptr, n, d_mm.ptr, 16,
                                                           n_blocks, None, best.ptr, ws.ptr, ws_bytes))
    assert np.array_equal(best.numpy(np.uint64), model.best(text, patterns, mm))
    gpu_ctx.near_scan_dev(None, 0, NO_SEP, None, None, 0, None, 16, 0, None, None, None, 0)      # n_patterns = 0 does nothing
