"""The three text scans (csrc/scan.hip, pattern.hip, near.hip) share their index and their tile loop (csrc/text_index.h), so on
inputs all three can express they must tell one story: fixed-length keys of W bytes, seed = block = W, max_mismatch = 0, no
separator. Through the device entries, with the text at a 16-byte-aligned and at an odd address, with whole and with 3-bit
hashes, each against its own brute-force model (window_scan_model.scan, pattern_scan_model.first_count, near_scan_model.best;
computed once per input and shared by the runs on it)."""
import functools

import numpy as np
import pytest

import dev_entry_checks as dev
import near_scan_model
import pattern_scan_model
import window_scan_model
from pangenomix_amd import _native

pytestmark = pytest.mark.gpu

NARROW = 1                                   # PGX_SCAN_NARROW_HASH == PGX_PATTERN_NARROW_HASH == PGX_NEAR_NARROW_HASH
ALPHABET = b'ACGT'
WIDTHS = (1, 16, 64)
N_KEYS = 300
# With 3 bits of hash every position is verified against every key, one key after the other: fewer keys keep that run short.
N_KEYS_NARROW = 48
NEAR_NONE = near_scan_model.NONE
NO_SEPARATOR = near_scan_model.NO_SEPARATOR


def tile():
    T = int(_native.lib().pgx_pattern_scan_tile())
    assert T == int(_native.lib().pgx_window_scan_tile()) == int(_native.lib().pgx_near_scan_tile())
    return T


def text_sizes(W):
    T = tile()
    return (W - 1, W, T, T + W - 1, T + W, 2 * T + W - 1)


@functools.lru_cache(maxsize=None)
def case(W, n_text, n_keys):
    """(text, keys, found, first, count, best): a text over ALPHABET and n_keys keys of W bytes -- every third one cut from the
    text (the first of them across the joint of the first two tiles, the second one ending with the text), some of them from a
    stretch that the text holds twice, every third one with a letter the text does not have, the others random -- and what the
    three models say of them."""
    rng = np.random.default_rng(1000 * W + n_text)
    T = tile()
    text = bytearray(pattern_scan_model.random_text(rng, n_text, ALPHABET))
    if n_text >= 4 * W:                                      # a stretch of 2 W bytes a second time, at the end of the text
        text[n_text - 2 * W:] = text[:2 * W]
    text = bytes(text)
    keys = []
    for k in range(n_keys):
        if k % 3 == 0 and n_text >= W:
            at = int(rng.integers(0, n_text - W + 1))
            if k == 0 and n_text >= T + W - 1:
                at = T - (W + 1) // 2                        # W > 1: it begins in the first tile and ends in the second
            elif k == 3:
                at = n_text - W
            elif k % 4 == 2:
                at = int(rng.integers(0, min(W, n_text - W) + 1))       # inside the stretch held twice, where there is one
            keys.append(text[at:at + W])
        elif k % 3 == 1:
            key = bytearray(pattern_scan_model.random_text(rng, W, ALPHABET))
            key[int(rng.integers(0, W))] = ord('N')
            keys.append(bytes(key))
        else:
            keys.append(pattern_scan_model.random_text(rng, W, ALPHABET))
    keys.append(keys[0])                                     # equal keys are all reported
    found = window_scan_model.scan(text, np.frombuffer(b''.join(keys), dtype=np.uint8), W) if n_text >= W else np.zeros(len(keys), np.uint8)
    first, count = pattern_scan_model.first_count(text, keys)
    best = near_scan_model.best(text, keys, np.zeros(len(keys), dtype=np.uint8))
    # the input is what it is meant to be
    if n_text >= W:
        assert found[0] and found[3] and found[-1] and found.sum() >= len(keys) // 3 and (found == 0).sum() >= len(keys) // 3
        if n_text >= T + W - 1 and W > 1:
            assert first[0] <= T - (W + 1) // 2 < T < T - (W + 1) // 2 + W
        if n_text >= 4 * W:
            assert (count >= 2).any()
    else:
        assert not found.any()
    return text, keys, found, first, count, best


def run_three(ctx, text, keys, W, flags, shift):
    """(found, first, count, best) of the three device entries on one copy of the text, `shift` bytes off 16-byte alignment"""
    lib = _native.lib()
    n = len(keys)
    data = np.frombuffer(text, dtype=np.uint8)
    key_rows = np.frombuffer(b''.join(keys), dtype=np.uint8)
    pb, po = pattern_scan_model.blob(keys)
    sizes = (int(lib.pgx_window_scan_workspace_bytes(data.size, n, W)), int(lib.pgx_pattern_workspace_bytes(pb.size, n)),
             int(lib.pgx_near_workspace_bytes(pb.size, n, n)))
    assert min(sizes) > 0 and sizes[0] == sizes[1] == sizes[2] - 16
    with dev.stream_scope('null') as stream:
        d_text = dev.guarded(shift + data.size, 0x5A)
        if data.size:
            d_text.raw[dev.GUARD + shift:dev.GUARD + shift + data.size] = dev.upload(data).dev
        assert d_text.ptr % 16 == 0
        d_keys, d_pb, d_po, d_mm = dev.upload(key_rows), dev.upload(pb), dev.upload(po), dev.upload(np.zeros(n, dtype=np.uint8))
        found, first, count, best = (dev.guarded(size * n, 0x5A) for size in (1, 4, 4, 8))
        workspaces = [dev.guarded(size, 0x5A) for size in sizes]
        with dev.unchanged(d_text.raw, d_keys, d_pb, d_po, d_mm):
            ctx.window_scan_dev(d_text.ptr + shift, data.size, d_keys.ptr, n, W, found.ptr, workspaces[0].ptr, sizes[0], flags,
                                stream)
            ctx.pattern_scan_dev(d_text.ptr + shift, data.size, d_pb.ptr, d_po.ptr, n, W, first.ptr, count.ptr,
                                 workspaces[1].ptr, sizes[1], flags, stream)
            ctx.near_scan_dev(d_text.ptr + shift, data.size, NO_SEPARATOR, d_pb.ptr, d_po.ptr, n, d_mm.ptr, W, n, None,
                              best.ptr, workspaces[2].ptr, sizes[2], flags, stream)
    for buf in [found, first, count, best] + workspaces:
        buf.assert_guards_intact()
    return found.numpy(np.uint8), first.numpy(np.uint32), count.numpy(np.uint32), best.numpy(np.uint64)


@pytest.mark.parametrize('flags', (0, NARROW))
@pytest.mark.parametrize('W', WIDTHS)
def test_the_three_scans_tell_one_story(W, flags, gpu_ctx):
    for n_text in text_sizes(W):
        text, keys, want_found, want_first, want_count, want_best = case(W, n_text, N_KEYS_NARROW if flags else N_KEYS)
        for shift in (0, 1):
            where = 'W %d, %d bytes of text, shift %d' % (W, n_text, shift)
            found, first, count, best = run_three(gpu_ctx, text, keys, W, flags, shift)
            # one story
            assert np.array_equal(found != 0, count > 0), where
            assert np.array_equal(found != 0, best != NEAR_NONE), where
            hit = found != 0
            assert np.array_equal(best[hit], first[hit].astype(np.uint64)), where     # (so the high word, the distance, is 0)
            # and the models'
            assert np.array_equal(found, want_found), where
            assert np.array_equal(first, want_first) and np.array_equal(count, want_count), where
            assert np.array_equal(best, want_best), where
