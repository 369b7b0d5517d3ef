"""The definition of pgx_term_scan in plain Python (include/pgx.h "Which of n_terms short patterns"): bytes.find on bytes
folded by a 256-entry table that maps A-Z to a-z and nothing else."""
import numpy as np

FOLD = 1                                     # PGX_TERM_FOLD_ASCII
_TABLE = bytes((b | 0x20) if 0x41 <= b <= 0x5A else b for b in range(256))


def fold(data, flags):
    return data.translate(_TABLE) if flags & FOLD else data


def blob(items, dtype=np.uint32):
    """(bytes uint8, offsets [n + 1]) of a list of byte strings laid end to end"""
    off = np.zeros(len(items) + 1, dtype=dtype)
    off[1:] = np.cumsum([len(x) for x in items])
    return np.frombuffer(b''.join(items), dtype=np.uint8), off


def windows(strings, lead=b''):
    """(text, start uint64, length uint32): the strings end to end behind `lead`"""
    text, off = blob(strings, np.uint64)
    start = off[:-1] + np.uint64(len(lead))
    length = np.array([len(s) for s in strings], dtype=np.uint32)
    return np.frombuffer(lead + text.tobytes(), dtype=np.uint8), start.astype(np.uint64), length


def masks(text, start, length, terms, flags):
    text = bytes(text)
    n_words = (len(terms) + 63) // 64
    out = np.zeros((len(start), n_words), dtype=np.uint64)
    folded = [fold(t, flags) for t in terms]
    for i, (s, n) in enumerate(zip(start.tolist(), length.tolist())):
        string = fold(text[s:s + n], flags)
        for t, term in enumerate(folded):
            if string.find(term) >= 0:
                out[i, t >> 6] |= np.uint64(1 << (t & 63))
    return out
