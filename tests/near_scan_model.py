"""The model of the bounded-mismatch pattern scan (csrc/near.hip; include/pgx.h "Bounded-mismatch search for variable-length
patterns"): the definition by brute force in numpy, every pattern against every window. It knows nothing of blocks or hashes,
and it is for small inputs only (text x pattern length bytes are compared per pattern)."""
import numpy as np

NONE = 0xFFFFFFFFFFFFFFFF
NO_SEPARATOR = 0x100


def best(text, patterns, max_mismatch, separator=NO_SEPARATOR, active=None):
    """uint64 [n]: min over the windows i of pattern k (i + L_k <= len(text), no `separator` byte in them) with d_k(i) <=
    max_mismatch[k] of d_k(i) << 32 | i; NONE for no such window and for a pattern whose active[k] is 0"""
    data = np.frombuffer(bytes(text), dtype=np.uint8)
    out = np.full(len(patterns), NONE, dtype=np.uint64)
    is_sep = np.concatenate([[0], np.cumsum(data == separator)]) if separator != NO_SEPARATOR else None
    memo = {}
    for k, p in enumerate(patterns):
        if active is not None and not active[k]:
            continue
        p, m = bytes(p), int(max_mismatch[k])
        if (p, m) not in memo:
            length, found = len(p), NONE
            if 0 < length <= data.size:
                windows = np.lib.stride_tricks.sliding_window_view(data, length)
                d = (windows != np.frombuffer(p, dtype=np.uint8)).sum(axis=1).astype(np.int64)
                ok = d <= m
                if is_sep is not None:
                    ok &= (is_sep[length:] - is_sep[:data.size - length + 1]) == 0
                if ok.any():
                    at = np.flatnonzero(ok)
                    i = at[np.argmin(d[at])]                                     # (argmin: the first of the smallest)
                    found = (int(d[i]) << 32) | int(i)
            memo[(p, m)] = found
        out[k] = memo[(p, m)]
    return out


def distance_and_position(value):
    return (int(value) >> 32, int(value) & 0xFFFFFFFF)


def mutate(window, places):
    """`window` with the bytes at `places` changed (xor 0x55: another byte value, never 0x00 for a letter)"""
    w = bytearray(window)
    for at in places:
        w[at] ^= 0x55
    return bytes(w)
