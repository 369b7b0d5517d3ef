"""TEST INFRASTRUCTURE: models of the window scan (csrc/scan.hip; include/pgx.h "Exact search for fixed-length keys") and of
the reference's direct UTR table validator (reference pangenome.py:1573-1647), plus the readers of tests/golden/proximal_direct.

  scan(text, keys, window)   found[k] = key k is one of the window-long slices of text: a Python set of slices
  validate_direct(...)       the reference's loop restated with str slicing, one iteration per base; what it prints is
                             appended to `out` line by line, so that the text printed before an exception is not lost
  ModelContext               stands in for a _native.Context in the host tests: window_scan() is scan()
  kernel_cases(window, n, T) texts and keys at the places where the kernel can go wrong"""
import collections
import json
import os

import numpy as np
import scipy.sparse

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
COMPLEMENT = str.maketrans('ACGTWSRYMKNacgtwsrymkn', 'TGCAWSYRKMNtgcawsyrkmn')


def scan(text, keys, window):
    text = bytes(np.asarray(text, dtype=np.uint8).tobytes()) if not isinstance(text, (bytes, bytearray)) else bytes(text)
    keys = np.ascontiguousarray(keys, dtype=np.uint8).reshape(-1, window)
    slices = {text[i:i + window] for i in range(len(text) - window + 1)}
    return np.array([k.tobytes() in slices for k in keys], dtype=np.uint8)


class ModelContext(object):
    def __init__(self):
        self.calls = []

    def window_scan(self, text, keys, flags=0):
        keys = np.asarray(keys)
        self.calls.append((bytes(text), keys.copy()))
        return scan(text, keys, keys.shape[1])


def read_fasta(path):
    out, name, blocks = {}, '', []
    for line in open(path):
        if line[0] == '>':
            if name and blocks:
                out[name] = ''.join(blocks)
            name, blocks = line.strip()[1:], []
        else:
            blocks.append(line.strip())
    if name and blocks:
        out[name] = ''.join(blocks)
    return out


def reverse_complement(seq):
    """KeyError of the first character that has no complement"""
    for base in seq:
        if ord(base) not in COMPLEMENT:
            raise KeyError(base)
    return seq.translate(COMPLEMENT)[::-1]


def validate_direct(index, columns, cells, genome_paths, nr_path, limits, side, log_group=1, out=None):
    """Returns the printed text. cells: (row, column) pairs of the present cells."""
    out = [] if out is None else out

    def say(*args):
        out.append(' '.join(str(a) for a in args) + '\n')
    say('Loading', side, 'sequences...')
    nr_prox = read_fasta(nr_path)
    window = limits[1] - limits[0]
    for g, fna in enumerate(genome_paths):
        contigs = read_fasta(fna)
        genome = os.path.splitext(os.path.split(fna)[1])[0]
        if (g + 1) % log_group == 0:
            say(g + 1, 'Evaluating', genome, fna)
        if genome not in columns:
            raise KeyError(genome)
        col = list(columns).index(genome)
        table_prox = [index[r] for r, c in sorted(cells) if c == col]
        seqs = {nr_prox[x]: x for x in table_prox}
        for contig in contigs.values():
            for i in range(len(contig)):
                seqs.pop(contig[i:i + window], None)
            rc = reverse_complement(contig)
            for i in range(len(rc)):
                seqs.pop(rc[i:i + window], None)
        for prox in seqs:
            say('\tMissing', seqs[prox], 'from', genome)
    if limits[1] >= 3 and side == 'upstream':
        say('Computing start codon distribution...')
        get = (lambda x: x[-3:]) if limits[1] == 3 else (lambda x: x[-limits[1]:-limits[1] + 3])
        say(collections.Counter(map(get, nr_prox.values())))
    elif limits[0] <= -3 and side == 'downstream':
        say('Computing stop codon distribution...')
        get = (lambda x: x[:3]) if limits[0] == -3 else (lambda x: x[-limits[0] - 3:-limits[0]])
        say(collections.Counter(map(get, nr_prox.values())))
    return ''.join(out)


# -- tests/golden/proximal_direct ------------------------------------------------------------------------------------------
def load_cases():
    with open(os.path.join(GOLDEN, 'proximal_direct', 'cases.json')) as f:
        return json.load(f)


def case_paths(case):
    return [os.path.join(GOLDEN, g) for g in case['genomes']], os.path.join(GOLDEN, case['nr'])


def case_frame(case):
    """the pandas frame the reference was given: NaN for absent cells"""
    import pandas as pd
    values = np.full((len(case['index']), len(case['columns'])), np.nan)
    for r, c in case['cells']:
        values[r, c] = 1.0
    return pd.DataFrame(values, index=case['index'], columns=case['columns'])


def case_lsdf(case):
    """the same table as build_upstream_pangenome returns it"""
    from pangenomix_amd import sparse_utils
    cells = np.asarray(case['cells'], dtype=np.int64).reshape(-1, 2)
    data = scipy.sparse.coo_matrix((np.ones(len(cells)), (cells[:, 0], cells[:, 1])),
                                   shape=(len(case['index']), len(case['columns'])))
    return sparse_utils.LightSparseDataFrame(np.asarray(case['index'], dtype=object), np.asarray(case['columns'], dtype=object),
                                             data)


def run_validator(fn, case, table, capsys, **kwargs):
    """(printed text with the golden directory written as <golden>, return value, exception or None) of
    fn(table, genomes, nr, **kwargs)"""
    genomes, nr = case_paths(case)
    capsys.readouterr()
    result = exc = None
    try:
        result = fn(table, genomes, nr, **kwargs)
    except Exception as e:              # compared with the recorded exception by the caller
        exc = e
    return capsys.readouterr().out.replace(GOLDEN, '<golden>'), result, exc


def assert_as_recorded(case, printed, result, exc):
    assert printed == case['stdout']
    if case['exception'] is None:
        assert exc is None, repr(exc)
        assert result == case['stdout'].count('\tMissing')
    else:
        assert exc is not None and type(exc).__name__ == case['exception']['type'] and exc.args[0] == case['exception']['arg']


# -- inputs for the kernel -------------------------------------------------------------------------------------------------
def kernel_case(window, text_bytes, tile, seed=0, alphabet=None):
    """(text uint8 [text_bytes], keys uint8 [n, window]): random text; keys that occur at position 0, end on the last byte and
    straddle every tile boundary at every offset from -(window - 1) to 0; each of those also with only its first and with
    only its last byte changed (near misses, unless the changed string occurs elsewhere -- the model decides); and random
    keys. An alphabet of 4 letters makes repeats and chance matches common, the default one uses all 256 byte values."""
    rng = np.random.default_rng(1000 * window + text_bytes + seed)
    letters = np.arange(256, dtype=np.uint8) if alphabet is None else np.frombuffer(alphabet, dtype=np.uint8)
    text = letters[rng.integers(0, letters.size, text_bytes)]
    n_pos = text_bytes - window + 1
    starts = set()
    if n_pos > 0:
        starts.update((0, n_pos - 1))
        for boundary in range(tile, text_bytes, tile):
            starts.update(s for s in range(boundary - (window - 1), boundary + 1) if 0 <= s < n_pos)
    keys = []
    for s in sorted(starts):
        key = text[s:s + window].copy()
        keys.append(key)
        for at in (0, window - 1):
            miss = key.copy()
            miss[at] ^= 0x20 if alphabet is not None else 0x01
            keys.append(miss)
    for _ in range(8):
        keys.append(letters[rng.integers(0, letters.size, window)])
    return text, np.array(keys, dtype=np.uint8).reshape(-1, window)
