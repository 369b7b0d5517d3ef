"""The model of the variable-length pattern scan (csrc/pattern.hip; include/pgx.h "Exact search for variable-length
patterns"): per pattern a bytes.find loop over the text gives the first position and the number of occurrences, overlapping
ones included. Also the blob layout the entries take and a generator of cases with planted patterns."""
import numpy as np

NONE = 0xFFFFFFFF


def first_count(text, patterns):
    """(first, count) uint32 [n]: the smallest i with text[i:i + len(p)] == p (NONE for none) and the number of such i"""
    text = bytes(text)
    first = np.full(len(patterns), NONE, dtype=np.uint32)
    count = np.zeros(len(patterns), dtype=np.uint32)
    memo = {}
    for k, p in enumerate(patterns):
        p = bytes(p)
        if p not in memo:
            at, n, lo = text.find(p), 0, NONE
            if at >= 0:
                lo = at
            while at >= 0:
                n += 1
                at = text.find(p, at + 1)
            memo[p] = (lo, n)
        first[k], count[k] = memo[p]
    return first, count


def blob(patterns, lead=0):
    """(uint8 blob, uint64 offsets [n + 1]) of the patterns end to end behind `lead` bytes that belong to no pattern"""
    lengths = np.array([len(p) for p in patterns], dtype=np.uint64)
    offsets = np.zeros(len(patterns) + 1, dtype=np.uint64)
    offsets[0] = lead
    np.cumsum(lengths, out=offsets[1:])
    offsets[1:] += np.uint64(lead)
    data = np.frombuffer(b'\xEE' * lead + b''.join(bytes(p) for p in patterns), dtype=np.uint8)
    return data, offsets


def random_text(rng, n, alphabet=None):
    if alphabet is None:
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    letters = np.frombuffer(alphabet, dtype=np.uint8)
    return letters[rng.integers(0, letters.size, n)].tobytes()


def kernel_case(rng, text_bytes, seed, alphabet=None, lengths=(), n_absent=4):
    """(text, patterns): a random text of text_bytes over `alphabet` (None: every byte value) and patterns of at least `seed`
    bytes -- for every length in `lengths` that fits one cut from a random place of the text and one from its very end, each
    with a copy whose last byte is changed; a pattern whose seed is the text's last `seed` bytes but whose tail runs past the
    text; one longer than the text; n_absent random ones."""
    text = random_text(rng, text_bytes, alphabet)
    patterns = []

    def near_miss(p):
        return p[:-1] + bytes([p[-1] ^ 0x01 if alphabet is None else alphabet[(alphabet.index(p[-1:]) + 1) % len(alphabet)]])
    for length in lengths:
        if seed <= length <= text_bytes:
            at = int(rng.integers(0, text_bytes - length + 1))
            for p in (text[at:at + length], text[text_bytes - length:]):       # anywhere; ending exactly at text_bytes
                patterns += [p, near_miss(p)]
    if text_bytes >= seed:
        patterns.append(text[text_bytes - seed:] + random_text(rng, 5, alphabet))          # its tail would run past the text
    patterns.append(text + random_text(rng, seed, alphabet))                                # longer than the text
    for _ in range(n_absent):
        patterns.append(random_text(rng, seed + int(rng.integers(0, 40)), alphabet))
    return text, patterns
