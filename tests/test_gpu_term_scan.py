"""Which terms occur in which strings on the device (csrc/terms.hip; include/pgx.h "Which of n_terms short patterns";
DESIGN.md 6n) against bytes.find (tests/terms_model.py). Bytes and bits: every comparison is exact. Everything runs with and
without PGX_TERM_FOLD_ASCII."""
import numpy as np
import pytest

import dev_entry_checks as dev
import terms_model as model
from pangenomix_amd import _native

pytestmark = pytest.mark.gpu

FLAGS = (0, model.FOLD)
MAX_TERMS, MAX_BYTES = _native.TERM_MAX_TERMS, _native.TERM_MAX_BYTES


def step():
    return int(_native.lib().pgx_term_scan_group_bytes())


def check(ctx, strings, terms, flags, lead=b''):
    text, start, length = model.windows(strings, lead)
    return check_windows(ctx, text, start, length, terms, flags)


def check_windows(ctx, text, start, length, terms, flags):
    blob, off = model.blob(terms)
    want = model.masks(text, start, length, terms, flags)
    got = ctx.term_scan(text, start, length, blob, off, flags)
    assert got.dtype == np.uint64 and got.shape == want.shape
    assert np.array_equal(got, want), 'masks differ in rows %r' % np.flatnonzero((got != want).any(axis=1))[:10].tolist()
    assert got.tobytes() == ctx.term_scan(text, start, length, blob, off, flags).tobytes()
    return got


def bit(mask, i, t):
    return bool((int(mask[i, t >> 6]) >> (t & 63)) & 1)


def random_strings(rng, alphabet, lengths):
    letters = np.frombuffer(alphabet, dtype=np.uint8)
    return [letters[rng.integers(0, letters.size, int(n))].tobytes() for n in lengths]


@pytest.mark.parametrize('flags', FLAGS)
def test_string_lengths_around_a_step(flags, gpu_ctx):
    G = step()
    assert G >= 16
    rng = np.random.default_rng(1)
    lengths = [0, 1, G - 1, G, G + 1, 4 * G + 3]
    strings = random_strings(rng, b'abAB', lengths * 4)
    terms = random_strings(rng, b'abAB', rng.integers(1, 5, 60)) + [s[-3:] for s in strings if len(s) >= 3] + [strings[1]]
    got = check(gpu_ctx, strings, terms, flags, lead=b'abab')
    assert got.any() and not got[0].any()


@pytest.mark.parametrize('flags', FLAGS)
def test_terms_at_the_edges_and_across_every_step_boundary(flags, gpu_ctx):
    """one planted term of 5 bytes in a string of 4G + 3 dots, at every place from 4 bytes before a boundary to the
    boundary itself, at the first byte and at the last"""
    G = step()
    n = 4 * G + 3
    places = sorted({0, n - 5} | {b - k for b in range(G, n, G) for k in range(5) if b - k + 5 <= n})
    strings = [b'.' * p + b'QwErT' + b'.' * (n - 5 - p) for p in places]
    terms = [b'QwErT', b'qwert', b'QwErTy', b'.QwErT.', b'wErT', b'T', b'Q.']
    got = check(gpu_ctx, strings, terms, flags)
    assert all(bit(got, i, 0) for i in range(len(strings)))
    assert all(bit(got, i, 1) == bool(flags) and not bit(got, i, 2) and bit(got, i, 5) for i in range(len(strings)))
    assert not bit(got, 0, 3) and not bit(got, len(strings) - 1, 3) and bit(got, 1, 3)


@pytest.mark.parametrize('flags', FLAGS)
def test_terms_longer_than_equal_to_and_inside_each_other(flags, gpu_ctx):
    strings = [b'', b'a', b'abc', b'abcabd', b'ABC', b'xabcx', b'ab']
    terms = [b'abc', b'abcd', b'ab', b'bc', b'b', b'abcabd', b'abcabda', b'cab', b'abd', b'a', b'c', b'bcab', b'ABC']
    got = check(gpu_ctx, strings, terms, flags)
    assert bit(got, 2, 0) and not bit(got, 2, 1) and not bit(got, 6, 0) and bit(got, 3, 5) and not bit(got, 3, 6)
    assert bit(got, 4, 0) == bool(flags)


@pytest.mark.parametrize('flags', FLAGS)
def test_the_empty_term(flags, gpu_ctx):
    strings = [b'', b'x', b'hello world']
    got = check(gpu_ctx, strings, [b''], flags)
    assert got[:, 0].tolist() == [1, 1, 1]
    terms = [b'x'] * 63 + [b'', b'hello', b'', b'y'] + [b'o w'] * 62 + [b'']
    got = check(gpu_ctx, strings, terms, flags)
    assert all(bit(got, i, t) for i in range(3) for t in (63, 65, 129)) and not bit(got, 0, 0)


@pytest.mark.parametrize('flags', FLAGS)
def test_200_terms_that_all_match_everywhere(flags, gpu_ctx):
    terms = [b'a' * k for k in range(1, 201)]
    strings = [b'a' * 4000, b'A' * 4000, b'a' * 150, b'a' * 199 + b'b' + b'a' * 200]
    got = check(gpu_ctx, strings, terms, flags)
    assert all(bit(got, 0, t) for t in range(200)) and bit(got, 2, 149) and not bit(got, 2, 150)
    assert bit(got, 3, 199) and bit(got, 1, 0) == bool(flags)


@pytest.mark.parametrize('flags', FLAGS)
def test_every_byte_value_and_the_neighbours_of_the_letters(flags, gpu_ctx):
    every = bytes(range(256))
    strings = [every, every[::-1], every * 2, b'@[`{', b'@AZ[', b'`az{', bytes([0xC1, 0xE1, 0xDA, 0xFA]), b'\x00\x00']
    strings += [b'@', b'[', b'\xc1', b'\xda', b'A', b'z']
    terms = [bytes([v]) for v in range(256)] + [bytes([v, (v + 1) & 255]) for v in range(0, 256, 3)]
    terms += [b'@', b'[', b'`', b'{', b'@a', b'z[', b'`A', b'Z{', b'\xc1', b'\xe1\xda', b'\xc1\xe1\xfa', b'\x00\x00\x00']
    got = check(gpu_ctx, strings, terms, flags)
    at = {t: i for i, t in enumerate(terms)}
    assert not bit(got, 3, at[b'@a']) and bit(got, 4, at[b'@a']) == bool(flags) and bit(got, 4, at[b'z[']) == bool(flags)
    assert bit(got, 5, at[b'`A']) == bool(flags) and bit(got, 5, at[b'Z{']) == bool(flags)
    for i, (a, b) in enumerate(((0x40, 0x60), (0x5B, 0x7B), (0xC1, 0xE1), (0xDA, 0xFA))):       # never folded onto each other
        assert bit(got, 8 + i, a) and not bit(got, 8 + i, b)
    assert bit(got, 12, 0x61) == bool(flags) and bit(got, 13, 0x5A) == bool(flags)            # 'A' holds 'a', 'z' holds 'Z'
    assert bit(got, 6, 0xC1) and bit(got, 6, 0xE1) and not bit(got, 6, at[b'\xc1\xe1\xfa'])
    assert not bit(got, 7, at[b'\x00\x00\x00']) and bit(got, 7, 0)


@pytest.mark.parametrize('flags', FLAGS)
@pytest.mark.parametrize('n_terms', (0, 1, 63, 64, 65, MAX_TERMS))
def test_term_counts(n_terms, flags, gpu_ctx):
    rng = np.random.default_rng(n_terms)
    strings = random_strings(rng, b'acgtAC', rng.integers(0, 150, 300))
    terms = random_strings(rng, b'acgtAC', rng.integers(1, 8, n_terms))
    if n_terms == MAX_TERMS:                                                     # and the limit of bytes, to the byte
        terms[-1] = strings[7][:50].ljust(MAX_BYTES - sum(len(t) for t in terms[:-1]), b'g')
        strings[8] = b'Tt' + terms[-1] + b'c'
        assert sum(len(t) for t in terms) == MAX_BYTES
    got = check(gpu_ctx, strings, terms, flags)
    assert got.shape == (300, (n_terms + 63) // 64)
    if n_terms:
        assert n_terms < 63 or got.any()
        if n_terms % 64:
            assert not (got[:, -1] >> np.uint64(n_terms % 64)).any()             # bits at and beyond n_terms
    if n_terms == MAX_TERMS:
        assert bit(got, 8, MAX_TERMS - 1) and not bit(got, 7, MAX_TERMS - 1)


@pytest.mark.parametrize('flags', FLAGS)
def test_no_strings_and_windows_that_overlap_or_repeat(flags, gpu_ctx):
    assert check(gpu_ctx, [], [b'a', b''], flags).shape == (0, 1)
    text = np.frombuffer(b'The quick brown fox jumps over the lazy dog', dtype=np.uint8)
    start = np.array([0, 4, 4, 10, 0, 43, 40, 16, 16], dtype=np.uint64)
    length = np.array([43, 5, 5, 9, 9, 0, 3, 3, 2], dtype=np.uint32)
    terms = [b'the', b'quick', b'brown fox', b'fox', b'fo', b'dog', b'k b', b'he qu']
    got = check_windows(gpu_ctx, text, start, length, terms, flags)
    assert np.array_equal(got[1], got[2]) and bit(got, 7, 3) and not bit(got, 8, 3) and bit(got, 8, 4)
    assert bit(got, 4, 0) == bool(flags) and bit(got, 0, 0)


@pytest.mark.parametrize('flags', FLAGS)
def test_20000_random_strings_against_100_random_terms(flags, gpu_ctx):
    rng = np.random.default_rng(20000)
    strings = random_strings(rng, b'acGT', rng.integers(0, 90, 20000))
    terms = random_strings(rng, b'acGT' if not flags else b'acgtACGT', rng.integers(1, 7, 100))
    got = check(gpu_ctx, strings, terms, flags, lead=b'\xff' * 5)
    assert 0.02 < np.unpackbits(got.view(np.uint8)).mean() < 0.6


def test_invalid_calls_are_refused_before_anything_is_written(gpu_ctx):
    lib, P, h = _native.lib(), _native._ptr, gpu_ctx._h
    text = np.frombuffer(b'abcdefgh', dtype=np.uint8)
    start, length = np.array([0, 4], dtype=np.uint64), np.array([4, 4], dtype=np.uint32)
    terms, off = model.blob([b'ab', b'gh'])
    out = np.full(2, 0x6E6E6E6E6E6E6E6E, dtype=np.uint64)

    def refused(rc, who):
        assert rc == -1, who                                                     # PGX_ERR_INVALID
        assert (out == 0x6E6E6E6E6E6E6E6E).all(), who

    def call(text_bytes=8, start=start, length=length, n=2, off=off, n_terms=2, flags=0):
        return lib.pgx_term_scan(h, P(text), text_bytes, P(start), P(length), n, P(terms), P(off), n_terms, flags, P(out))
    refused(call(n=1 << 24), 'n')
    refused(call(text_bytes=1 << 32), 'text_bytes')
    refused(call(start=np.array([0, 5], dtype=np.uint64)), 'a window that leaves the text')
    refused(call(start=np.array([0, 9], dtype=np.uint64), length=np.array([4, 0], dtype=np.uint32)), 'a window behind the text')
    refused(call(length=np.array([4, 0xFFFFFFFF], dtype=np.uint32)), 'a window that wraps')
    refused(call(flags=2), 'unknown flags')
    refused(call(n_terms=MAX_TERMS + 1), 'too many terms')
    refused(call(off=np.array([0, 3, 2], dtype=np.uint32)), 'decreasing offsets')
    refused(call(off=np.array([0, 2, MAX_BYTES + 1], dtype=np.uint32)), 'too many term bytes')
    assert call() == 0 and out.tolist() == [1, 2]
    g = dev.guarded(4096, 0x5A)
    for n, text_bytes, n_terms, term_bytes, flags in ((1 << 24, 8, 2, 4, 0), (2, 1 << 32, 2, 4, 0), (2, 8, MAX_TERMS + 1, 4, 0),
                                                      (2, 8, 2, MAX_BYTES + 1, 0), (2, 8, 2, 4, 4)):
        with pytest.raises(_native.PgxError) as e:
            gpu_ctx.term_scan_dev(g.ptr, text_bytes, g.ptr, g.ptr, n, g.ptr, g.ptr, n_terms, term_bytes, g.ptr, flags)
        assert e.value.status == -1
    assert g.is_still_garbage()
    g.assert_guards_intact()


# -- the device entry ------------------------------------------------------------------------------------------------------
def dev_case(seed, n, n_terms):
    rng = np.random.default_rng(seed)
    strings = random_strings(rng, b'abAB.', rng.integers(0, 3 * step(), n))
    terms = random_strings(rng, b'abAB.', rng.integers(0, 6, n_terms))
    return model.windows(strings, b'..') + model.blob(terms) + (terms,)


def run_dev(ctx, case, flags, fill, stream):
    text, start, length, blob, off, terms = case
    n_words = (len(terms) + 63) // 64
    with dev.stream_scope(stream) as handle:
        d_text, d_start, d_len, d_blob, d_off = (dev.upload(x) for x in (text, start, length, blob, off))
        out = dev.guarded(8 * start.size * n_words, fill)
        with dev.unchanged(d_text, d_start, d_len, d_blob, d_off):
            ctx.term_scan_dev(d_text.ptr, text.size, d_start.ptr, d_len.ptr, start.size, d_blob.ptr, d_off.ptr, len(terms),
                              blob.size, out.ptr, flags, handle)
    out.assert_guards_intact()
    return (out.numpy(np.uint64).reshape(start.size, n_words),)


@pytest.mark.parametrize('flags', FLAGS)
@pytest.mark.parametrize('stream', dev.STREAMS)
def test_device_entry_on_caller_tensors(stream, flags, gpu_ctx):
    for seed, n, n_terms in ((1, 500, 70), (2, 1, 1), (3, 17, 64)):
        case = dev_case(seed, n, n_terms)
        want = model.masks(case[0], case[1], case[2], case[5], flags)
        per_fill = []
        for fill in dev.FILLS:
            got = run_dev(gpu_ctx, case, flags, fill, stream)
            assert np.array_equal(got[0], want)
            per_fill.append(got)
        dev.same_bytes(per_fill)


def test_device_entry_clamps_windows_into_the_text(gpu_ctx):
    """the device entry does not look at the windows: one that leaves the text is cut short at its end"""
    text = np.frombuffer(b'abcdefgh', dtype=np.uint8)
    start, length = np.array([6, 8, 1 << 40, 0], dtype=np.uint64), np.array([100, 5, 5, 0xFFFFFFFF], dtype=np.uint32)
    terms = [b'gh', b'h', b'', b'abcdefgh', b'ghi']
    blob, off = model.blob(terms)
    got, = run_dev(gpu_ctx, (text, start, length, blob, off, terms), 0, 0x5A, 'null')
    assert got[:, 0].tolist() == [0b00111, 0b00100, 0b00100, 0b01111]


def test_device_entry_does_not_allocate(gpu_ctx):
    text, start, length, blob, off, terms = dev_case(4, 500, 70)
    d_text, d_start, d_len, d_blob, d_off = (dev.upload(x) for x in (text, start, length, blob, off))
    out = dev.guarded(8 * start.size * 2, 0xFF)
    dev.assert_no_allocation(lambda: gpu_ctx.term_scan_dev(d_text.ptr, text.size, d_start.ptr, d_len.ptr, start.size, d_blob.ptr,
                                                           d_off.ptr, len(terms), blob.size, out.ptr))
