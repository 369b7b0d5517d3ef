"""pangenomix_amd.mlst.host_near -- the block rule of the bounded-mismatch scan on the host (bytes.find per distinct block, a
numpy compare of the windows it names) -- against the brute-force model (tests/near_scan_model.py): the cases of
tests/test_gpu_near_scan.py that need no device."""
import numpy as np
import pytest

import near_scan_model as model
from pattern_scan_model import random_text
from pangenomix_amd import mlst

NONE = model.NONE


def check(text, patterns, mm, block, separator=model.NO_SEPARATOR, active=None):
    got = mlst.host_near(text, patterns, mm, block, separator=separator, active=active)
    want = model.best(text, patterns, mm, separator, active)
    assert got.dtype == np.uint64 and np.array_equal(got, want), np.flatnonzero(got != want)[:10].tolist()
    return got


def one_per_block(block, blocks):
    return [j * block + (5 * j + 3) % block for j in blocks]


def test_constants_agree():
    assert mlst.NEAR_NONE == model.NONE and mlst.NEAR_NO_SEPARATOR == model.NO_SEPARATOR


@pytest.mark.parametrize('block', (1, 8, 13, 19, 32, 64))
def test_text_sizes(block):
    B, T = block, 700
    rng = np.random.default_rng(B)
    found = 0
    for n in sorted({0, B - 1, B, B + 1, T - 1, T, T + 1, 2 * T + B - 2}):
        text = random_text(rng, n)
        patterns, mm = [text + random_text(rng, B), random_text(rng, 3 * B)], [0, 2]
        for length in (B, B + 1, 3 * B, 70, 200):
            m = min(2, length // B - 1)
            if B <= length <= n:
                for at in (int(rng.integers(0, n - length + 1)), n - length):
                    window = text[at:at + length]
                    for d in (m, m + 1):
                        patterns.append(model.mutate(window, sorted(rng.choice(length, size=d, replace=False).tolist())))
                        mm.append(m)
        best = check(text, patterns, mm, B)
        assert best[0] == NONE
        found += int((best != NONE).sum())
    assert found > 10


@pytest.mark.parametrize('m,block,length', ((0, 13, 50), (1, 13, 50), (2, 13, 50), (22, 19, 450), (255, 4, 1100), (255, 1, 700)))
def test_distance_exactly_m_is_found_and_m_plus_one_is_not(m, block, length):
    rng = np.random.default_rng(m)
    p_in, p_out = random_text(rng, length, b'ACGT'), random_text(rng, length, b'ACGT')
    text = bytearray(random_text(rng, 2 * length + 400, b'ACGT'))
    text[100:100 + length] = model.mutate(p_in, one_per_block(block, range(m)))
    text[length + 200:2 * length + 200] = model.mutate(p_out, one_per_block(block, range(m + 1)))
    assert check(bytes(text), [p_in, p_out], [m, m], block).tolist() == [(m << 32) | 100, NONE]


def test_every_block_index_leads_to_the_window():
    L, m, B = 450, 22, 19
    rng = np.random.default_rng(23)
    patterns = [random_text(rng, L, b'ACGT') for _ in range(m + 1)]
    text = bytearray(random_text(rng, 60 + (m + 1) * 520, b'ACGT'))
    for j in range(m + 1):
        at = 31 + j * 520
        text[at:at + L] = model.mutate(patterns[j], one_per_block(B, [b for b in range(m + 1) if b != j]))
    best = check(bytes(text), patterns, [m] * (m + 1), B)
    assert best.tolist() == [(m << 32) | (31 + j * 520) for j in range(m + 1)]


def test_windows_at_the_ends_of_the_text():
    B, m = 13, 3
    rng = np.random.default_rng(31)
    p = random_text(rng, 60, b'ACGT')
    for j in (1, 2, 3):
        assert (check(p[j * B:] + random_text(rng, 300, b'ACGT'), [p], [m], B) == NONE).all()
    text = random_text(rng, 500, b'ACGT') + model.mutate(p, [5, 20])
    past = text[len(text) - 59:] + b'A'
    assert check(text, [p, past, past[:59]], [m, m, m], B).tolist() == [(2 << 32) | 500, NONE, len(text) - 59]


@pytest.mark.parametrize('separator', (0, ord('N')))
def test_separator_ties_and_active(separator):
    B, m = 13, 1
    rng = np.random.default_rng(41)
    sep = bytes([separator])
    p_clean, p_holds = random_text(rng, 50, b'ACGT'), random_text(rng, 20, b'ACGT') + sep + random_text(rng, 29, b'ACGT')
    text = bytearray(random_text(rng, 3000, b'ACGT'))
    text[100:150] = p_clean[:30] + sep + p_clean[31:]
    text[300:350] = p_holds
    text[2000:2050] = model.mutate(p_clean, [7])
    text[2500:2550] = model.mutate(p_clean, [8])
    text = bytes(text)
    assert check(text, [p_clean, p_holds], [m, m], B, separator=separator).tolist() == [(1 << 32) | 2000, NONE]
    assert check(text, [p_clean, p_holds], [m, m], B).tolist() == [(1 << 32) | 100, 300]
    assert check(text, [p_clean, p_holds], [m, m], B, active=[0, 1]).tolist() == [NONE, 300]
    assert check(text, [p_clean, p_holds], [m, m], B, active=[0, 0]).tolist() == [NONE, NONE]


def test_a_pattern_too_short_for_its_blocks_is_refused():
    with pytest.raises(ValueError, match='shorter'):
        mlst.host_near(b'ACGTACGTACGT', [b'ACGTAC'], [1], 4)
