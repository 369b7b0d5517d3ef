"""TEST INFRASTRUCTURE: references for the local alignment of DESIGN.md 6t that share no code with the model ncbi.host_sw or
with csrc/sw.hip -- a score-only Smith-Waterman and a full-matrix traceback with the same tie rules -- and the sequence
builders that the host tests (test_ncbi_host.py) and the GPU tests of test_gpu_sw_rounds.py share. Nothing here needs a GPU."""
import numpy as np

from pangenomix_amd import ncbi

NEG = -10 ** 9
CORE_LETTERS = np.frombuffer(b'ACDEFGHIKLMNQRSTVY', dtype=np.uint8)        # no W, no P: the flanks of the tests match nothing
AA20 = np.frombuffer(b'ACDEFGHIKLMNPQRSTVWY', dtype=np.uint8)

_by_byte = None


def sub(a, b):
    """substitution score of two one-byte sequences: ncbi.tables() over ncbi.letters_of, looked up by byte"""
    global _by_byte
    if _by_byte is None:
        letters = ncbi.letters_of(np.arange(256, dtype=np.uint8))
        _by_byte = ncbi.tables()[1][letters][:, letters].tolist()
    return _by_byte[a[0]][b[0]]


def self_score(s):
    return sum(sub(s[i:i + 1], s[i:i + 1]) for i in range(len(s)))


def core(n, seed):
    return CORE_LETTERS[np.random.default_rng(seed).integers(0, CORE_LETTERS.size, n)].tobytes()


def pack(seqs):
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return np.frombuffer(b''.join(bytes(s) for s in seqs), dtype=np.uint8), off


def score_only(q, s):
    """best score and its first cell, row by row"""
    best, H, F = (0, 0, 0), [0] * (len(s) + 1), [NEG] * (len(s) + 1)
    for i in range(len(q)):
        diag, left, E = 0, 0, NEG
        for j in range(len(s)):
            E = max(E - 1, left - 12)
            F[j + 1] = max(F[j + 1] - 1, H[j + 1] - 12)
            left, diag = max(0, diag + sub(q[i:i + 1], s[j:j + 1]), E, F[j + 1]), H[j + 1]
            H[j + 1] = left
            if left > best[0]:
                best = (left, i, j)
    return best


def traceback_sw(q, s):
    """The eight values by full matrices and a traceback: extension before opening, the diagonal before E, E before F."""
    m, n = len(q), len(s)
    H = np.zeros((m + 1, n + 1), dtype=np.int64)
    E, F = np.full((m + 1, n + 1), NEG, dtype=np.int64), np.full((m + 1, n + 1), NEG, dtype=np.int64)
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            E[i, j] = max(E[i, j - 1] - 1, H[i, j - 1] - 12)
            F[i, j] = max(F[i - 1, j] - 1, H[i - 1, j] - 12)
            H[i, j] = max(0, H[i - 1, j - 1] + sub(q[i - 1:i], s[j - 1:j]), E[i, j], F[i, j])
    best = int(H.max())
    if best == 0:
        return [0] * 8
    i, j = [int(x) for x in np.argwhere(H == best)[0]]                    # row-major: the smallest i, then the smallest j
    end = (i - 1, j - 1)
    state, ident, cols, gaps = 'H', 0, 0, 0
    while True:
        if state == 'H':
            d = H[i - 1, j - 1] + sub(q[i - 1:i], s[j - 1:j])
            if d >= E[i, j] and d >= F[i, j]:
                cols += 1
                ident += ncbi.letters_of(q[i - 1:i])[0] == ncbi.letters_of(s[j - 1:j])[0]
                if H[i - 1, j - 1] == 0:
                    return [best, i - 1, end[0], j - 1, end[1], int(ident), cols, gaps]
                i, j = i - 1, j - 1
            else:
                state = 'E' if E[i, j] >= F[i, j] else 'F'
        elif state == 'E':
            cols += 1
            if not E[i, j - 1] - 1 >= H[i, j - 1] - 12:
                gaps += 1
                state = 'H'
            j -= 1
        else:
            cols += 1
            if not F[i - 1, j] - 1 >= H[i - 1, j] - 12:
                gaps += 1
                state = 'H'
            i -= 1


def random_pairs(count, letters, longest, seed):
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(letters, dtype=np.uint8)
    return [tuple(letters[rng.integers(0, letters.size, int(n))].tobytes() for n in rng.integers(1, longest + 1, 2))
            for _ in range(count)]


def two_letter_relatives(count=8, seed=41):
    """(q, s) pairs over the letters A and C, q of 66..140 residues (past one strip of the kernel), s = q without a planted
    block of 1..5 residues at least 30 from either end: with two letters equal scores are everywhere, and the flanks of 30
    identities (4 or 9 each) outweigh a gap of at most 11 + 5, so the best alignment is gapped."""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b'AC', dtype=np.uint8)
    pairs = []
    for _ in range(count):
        n, k = int(rng.integers(66, 141)), int(rng.integers(1, 6))
        q = letters[rng.integers(0, 2, n)].tobytes()
        cut = int(rng.integers(30, n - 30 - k + 1))
        pairs.append((q, q[:cut] + q[cut + k:]))
    return pairs
