"""TEST INFRASTRUCTURE: models of the exact dictionary match (csrc/dict.hip; include/pgx.h "Exact look-up of whole byte
strings") and of the reference's table-against-FASTA validator (reference pangenome.py:1418-1546), plus the readers of
tests/golden/table_fasta.

  first_last(keys, queries)   first[k] / last[q] from a Python dict of bytes objects
  sets_diff(...)              the two counts per genome from numpy sets of (row, genome) pairs
  validate(...)               the reference's validator restated statement by statement, hashlib.sha256 and all; what it
                              prints is appended to `out` line by line, so the text printed before an exception is not lost
  ModelContext                stands in for a _native.Context in the host tests: dict_load / dict_query / genome_sets_diff
  blob(strings, lead)         (blob, offsets) of a list of bytes objects, `lead` unused bytes in front"""
import hashlib
import json
import os

import numpy as np
import scipy.sparse

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


# -- the kernels -----------------------------------------------------------------------------------------------------------
def blob(strings, lead=0):
    offsets = np.zeros(len(strings) + 1, dtype=np.uint64)
    offsets[0] = lead
    if strings:
        offsets[1:] = lead + np.cumsum([len(s) for s in strings], dtype=np.uint64)
    return np.frombuffer(b'\xEE' * lead + b''.join(strings), dtype=np.uint8), offsets


def strings_of(data, offsets):
    data = bytes(np.asarray(data, dtype=np.uint8).tobytes())
    offsets = [int(x) for x in offsets]
    return [data[offsets[i]:offsets[i + 1]] for i in range(len(offsets) - 1)]


def first_last(keys, queries):
    """keys, queries: lists of bytes. first int32 [n_keys], last int32 [n_queries]."""
    first_of, last_of = {}, {}
    for k, key in enumerate(keys):
        first_of.setdefault(key, k)
        last_of[key] = k
    return (np.array([first_of[key] for key in keys], dtype=np.int32).reshape(-1),
            np.array([last_of.get(q, -1) for q in queries], dtype=np.int32).reshape(-1))


def sets_diff(a_rows, a_genomes, b_rows, b_genomes, n_rows, n_genomes):
    a = set(zip(np.asarray(a_rows).tolist(), np.asarray(a_genomes).tolist()))
    b = set(zip(np.asarray(b_rows).tolist(), np.asarray(b_genomes).tolist()))
    assert all(0 <= r < n_rows and 0 <= g < n_genomes for r, g in a | b)
    a_only, b_only = np.zeros(n_genomes, dtype=np.uint32), np.zeros(n_genomes, dtype=np.uint32)
    for _, g in a - b:
        a_only[g] += 1
    for _, g in b - a:
        b_only[g] += 1
    return a_only, b_only


class ModelContext(object):
    def __init__(self):
        self.keys = None
        self.loads, self.queries, self.diffs = 0, [], 0

    def dict_load(self, keys, key_offsets, flags=0, want_first=True):
        self.keys = strings_of(keys, key_offsets)
        self.loads += 1
        return first_last(self.keys, [])[0]

    def dict_query(self, queries, query_offsets):
        assert self.keys is not None
        queries = strings_of(queries, query_offsets)
        self.queries.append(len(queries))
        return first_last(self.keys, queries)[1]

    def genome_sets_diff(self, a_rows, a_genomes, b_rows, b_genomes, n_rows, n_genomes):
        self.diffs += 1
        return sets_diff(a_rows, a_genomes, b_rows, b_genomes, n_rows, n_genomes)


# -- the reference's validator, restated -----------------------------------------------------------------------------------
def trim_variant(feature_name):
    for i in range(1, len(feature_name)):
        if feature_name[-i].isalpha():
            return feature_name[:-i]
    return feature_name


def sha(text):
    return hashlib.sha256(text.encode('utf-8')).digest()


def validate(index, columns, cells, genome_paths, nr_path, allele_names=None, log_group=1, out=None):
    """index / columns: the table's labels; cells: {(row, column): value}, a missing cell being NaN. Returns the printed
    text; raises what the reference raises."""
    out = [] if out is None else out

    def say(*args):
        out.append(' '.join(str(a) for a in args) + '\n')
    inconsistencies = 0
    if allele_names:
        say('Loading feature names...')
        feathash_to_allele = {}
        with open(allele_names, 'r') as f:
            for line in f:
                data = line.strip().split('\t')
                allele = data[0]
                for feature in data[1:]:
                    if feature.count('|') == 2:
                        feature = feature[:feature.rindex('|')]
                    feathash_to_allele[sha(feature)] = allele
    say('Loading non-redundant sequences...')
    seqhash_to_feature = {}

    def load_sequence_entry(seq_blocks, header):
        if len(seq_blocks) > 0:
            seq = ''.join(seq_blocks)
            seq = seq if (allele_names is None) else seq + trim_variant(header)
            seqhash = sha(seq)
            if seqhash in seqhash_to_feature:
                say('COLLISION:', header)
            seqhash_to_feature[seqhash] = header
    with open(nr_path, 'r') as f_fasta:
        header, seq_blocks = '', []
        for line in f_fasta:
            if line[0] == '>':
                load_sequence_entry(seq_blocks, header)
                header = line[1:].strip()
                seq_blocks = []
            else:
                seq_blocks.append(line.strip())
        load_sequence_entry(seq_blocks, header)
    say('Non-redundant sequences:', len(seqhash_to_feature))

    def check_genome_sequence(seq_blocks, genome_features, feature_name):
        if len(seq_blocks) > 0:
            seq = ''.join(seq_blocks)
            if not (allele_names is None):
                feature_name = feature_name.split('_upstream(')[0]
                feature_name = feature_name.split('_downstream(')[0]
                feature_hash = sha(feature_name)
                if feature_hash in feathash_to_allele:
                    seq += trim_variant(feathash_to_allele[feature_hash])
            seqhash = sha(seq)
            if seqhash in seqhash_to_feature:
                genome_features.add(seqhash_to_feature[seqhash])
        return genome_features
    missing_features = 0
    for i, genome_fasta in enumerate(sorted(genome_paths)):
        if (i + 1) % log_group == 0:
            say('Validating genome', i + 1, ':', genome_fasta)
        genome_features = set()
        with open(genome_fasta, 'r') as f_fasta:
            feature_header, seq_blocks = '', []
            for line in f_fasta:
                if line[0] == '>':
                    genome_features = check_genome_sequence(seq_blocks, genome_features, feature_header)
                    feature_header = line[1:].strip()
                    seq_blocks = []
                else:
                    seq_blocks.append(line.strip())
            genome_features = check_genome_sequence(seq_blocks, genome_features, feature_header)
        genome = os.path.splitext(os.path.split(genome_fasta)[1])[0]
        if genome not in columns:
            genome = '_'.join(genome.split('_')[:-1])
        if genome not in columns:
            raise KeyError(genome)
        col = list(columns).index(genome)
        table_features = set(index[r] for (r, c), v in cells.items() if c == col and v == 1)
        test = table_features == genome_features
        inconsistencies += (1 - int(test))
        if not test:
            say(genome, '\t', 'Table only:', len(table_features.difference(genome_features)), '\t', 'Genome only:',
                len(genome_features.difference(table_features)))
    say('Missing Features:', missing_features)
    say('Feature Table Inconsistencies:', inconsistencies)
    return ''.join(out)


# -- tests/golden/table_fasta ----------------------------------------------------------------------------------------------
def load_cases():
    """every case with a whole table: index, columns, cells (a case recorded against a named table has that table's
    labels and cells, the labels appended to its index, the cells added and removed)"""
    with open(os.path.join(GOLDEN, 'table_fasta', 'cases.json')) as f:
        data = json.load(f)
    cases = data['cases']
    for case in cases.values():
        if case['table'] is not None:
            table = data['tables'][case['table']]
            cells = (set(map(tuple, table['cells'])) - set(map(tuple, case['cells_removed']))) | set(map(tuple, case['cells_added']))
            case.update(index=table['index'] + case['index_appended'], columns=table['columns'],
                        cells=[list(x) for x in sorted(cells)])
    return cases


def case_paths(case):
    names = os.path.join(GOLDEN, case['allele_names']) if case['allele_names'] else None
    return [os.path.join(GOLDEN, g) for g in case['genomes']], os.path.join(GOLDEN, case['nr']), names


def case_cells(case):
    """{(row, column): value}: the present cells are 1; `other` holds the cells with any other value (None = NaN)"""
    cells = {(r, c): 1 for r, c in case['cells']}
    for r, c, v in case['other']:
        cells[(r, c)] = float('nan') if v is None else v
    return cells


def is_binary(case):
    """a table an LSDF can hold: no cell with a value other than 1"""
    return not case['other']


def case_frame(case):
    """the pandas frame the reference was given: 0 for absent cells, `other` as recorded"""
    import pandas as pd
    values = np.zeros((len(case['index']), len(case['columns'])))
    for (r, c), v in case_cells(case).items():
        values[r, c] = v
    return pd.DataFrame(values, index=case['index'], columns=case['columns'])


def case_lsdf(case):
    from pangenomix_amd import sparse_utils
    assert is_binary(case)
    cells = np.asarray(case['cells'], dtype=np.int64).reshape(-1, 2)
    data = scipy.sparse.coo_matrix((np.ones(len(cells)), (cells[:, 0], cells[:, 1])),
                                   shape=(len(case['index']), len(case['columns'])))
    return sparse_utils.LightSparseDataFrame(np.asarray(case['index'], dtype=object), np.asarray(case['columns'], dtype=object),
                                             data)


def run_validator(fn, case, table, capsys, **kwargs):
    """(printed text with the golden directory written as <golden>, return value, exception or None) of the validator `fn`
    called the way the case's kind asks for"""
    genomes, nr, names = case_paths(case)
    capsys.readouterr()
    result = exc = None
    try:
        if names is None:
            result = fn(table, genomes, nr, log_group=case['log_group'], **kwargs)
        else:
            result = fn(table, genomes, nr, names, log_group=case['log_group'], **kwargs)
    except Exception as e:              # compared with the recorded exception by the caller
        exc = e
    return capsys.readouterr().out.replace(GOLDEN, '<golden>'), result, exc


def recorded_count(case):
    return int(case['stdout'].rsplit('Feature Table Inconsistencies: ', 1)[1]) if case['exception'] is None else None


def assert_as_recorded(case, printed, result, exc):
    assert printed == case['stdout']
    if case['exception'] is None:
        assert exc is None, repr(exc)
        assert result == recorded_count(case)
    else:
        assert exc is not None and type(exc).__name__ == case['exception']['type'] and exc.args[0] == case['exception']['arg']
