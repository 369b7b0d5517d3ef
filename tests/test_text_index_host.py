"""The workspace sizes of the three text scans (csrc/text_index.h make_geom), pinned to their closed form: device callers size
their buffers by these values, so they are part of the ABI. No device is needed: the library only computes."""
import pytest

from pangenomix_amd import _native

FILTER_BYTES = 32768                  # 2^18 bits
TICKET_BYTES = 16                     # near's tail


def closed_form(n):
    slots = 64
    while slots < 2 * n:
        slots *= 2
    return slots * 8 + FILTER_BYTES


def window_bytes(n, text_bytes=1000, window=32):
    return int(_native.lib().pgx_window_scan_workspace_bytes(text_bytes, n, window))


def pattern_bytes(n, blob_bytes=1000):
    return int(_native.lib().pgx_pattern_workspace_bytes(blob_bytes, n))


def near_bytes(n_blocks, blob_bytes=1000, n_patterns=10):
    return int(_native.lib().pgx_near_workspace_bytes(blob_bytes, n_patterns, n_blocks))


@pytest.mark.parametrize('n, want', [(0, 33280), (1, 33280), (32, 33280), (33, 33792), (2 ** 24 - 1, 2 ** 25 * 8 + 32768)])
def test_workspace_bytes_are_the_closed_form(n, want):
    assert closed_form(n) == want
    assert window_bytes(n) == want
    assert pattern_bytes(n) == want
    assert near_bytes(n) == want + TICKET_BYTES


@pytest.mark.parametrize('n', [2, 31, 64, 65, 1000, 4200, 96600, 2 ** 20, 2 ** 20 + 1])
def test_workspace_bytes_between_the_pinned_sizes(n):
    assert window_bytes(n) == pattern_bytes(n) == near_bytes(n) - TICKET_BYTES == closed_form(n)


def test_near_is_sized_by_blocks_not_patterns():
    assert near_bytes(2 ** 30 - 1, n_patterns=1) == 2 ** 31 * 8 + FILTER_BYTES + TICKET_BYTES
    assert near_bytes(33, n_patterns=2 ** 24 - 1) == 33792 + TICKET_BYTES


def test_refusals_return_zero():
    assert window_bytes(2 ** 24) == 0 and pattern_bytes(2 ** 24) == 0
    assert near_bytes(10, n_patterns=2 ** 24) == 0
    assert window_bytes(10, text_bytes=2 ** 32) == 0
    assert pattern_bytes(10, blob_bytes=2 ** 32) == 0
    assert near_bytes(10, blob_bytes=2 ** 32) == 0
    assert near_bytes(2 ** 30) == 0
    assert window_bytes(10, window=0) == 0 and window_bytes(10, window=1025) == 0
    # the last sizes that are accepted
    assert window_bytes(10, text_bytes=2 ** 32 - 1, window=1024) == closed_form(10)
    assert window_bytes(10, window=1) == closed_form(10)
    assert pattern_bytes(10, blob_bytes=2 ** 32 - 1) == closed_form(10)
