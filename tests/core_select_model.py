"""TEST INFRASTRUCTURE: a plain-numpy restatement (one thread, plain loops) of the outputs of pgx_core_select
(include/pgx.h, "Core / dominant allele selection"; pangenomix_amd/csrc/select.hip) from DENSE 0/1 tables,
the reader of tests/golden/core_fasta, and a stand-in context for the host tests. tests/test_core_fasta_host.py checks
the model against the selections the reference made on every fixture, so it is a fair yardstick for the sizes no fixture
covers.

    gene_count[r]   = G[gene_of_run[r]].sum() if there is a gene table and gene_of_run[r] >= 0, else 0
    best_allele[r]  = first row of run r with the largest count (-1 for an empty run), best_count[r] that count
    eligible[r]     = best_allele[r] >= 0 and (gene_of_run is None or gene_of_run[r] >= 0)
    mask[r] bit t   = eligible[r] and gene_count[r] >= thresholds[t]
    selected[t]     = [best_allele[r] for r in ascending order if mask[r] bit t], n_selected[t] its length
"""
import json
import os

import numpy as np

import allele_runs_model

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'core_fasta')
CDS = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'cds', 'expected')
OUTPUTS = ('gene_count', 'best_allele', 'best_count', 'mask', 'selected', 'n_selected')


def select(A, run_start, thresholds, G=None, gene_of_run=None):
    """dict of the six outputs; 'selected' is a list of n_thresholds int32 arrays."""
    A = np.asarray(A, dtype=bool)
    run_start = [int(x) for x in run_start]
    thresholds = [int(x) for x in thresholds]
    n_runs = len(run_start) - 1
    counts = A.sum(axis=1, dtype=np.int64)
    gene_count = np.zeros(n_runs, dtype=np.uint32)
    best_allele = np.full(n_runs, -1, dtype=np.int32)
    best_count = np.zeros(n_runs, dtype=np.uint32)
    mask = np.zeros(n_runs, dtype=np.uint32)
    selected = [[] for _ in thresholds]
    for r in range(n_runs):
        for i in range(run_start[r], run_start[r + 1]):
            if best_allele[r] < 0 or counts[i] > best_count[r]:
                best_allele[r], best_count[r] = i, counts[i]
        eligible = best_allele[r] >= 0
        if gene_of_run is not None:
            eligible = eligible and int(gene_of_run[r]) >= 0
            if G is not None and int(gene_of_run[r]) >= 0:
                gene_count[r] = int(np.asarray(G, dtype=bool)[int(gene_of_run[r])].sum())
        for t, x in enumerate(thresholds):
            if eligible and int(gene_count[r]) >= x:
                mask[r] |= np.uint32(1 << t)
                selected[t].append(int(best_allele[r]))
    return {'gene_count': gene_count, 'best_allele': best_allele, 'best_count': best_count, 'mask': mask,
            'selected': [np.asarray(s, dtype=np.int32) for s in selected],
            'n_selected': np.asarray([len(s) for s in selected], dtype=np.uint32)}


def assert_equal(got, want, keys=None):
    """Exact equality, dtypes included, of a result dict with the model's (over `keys`, default: what got holds)."""
    for k in (keys if keys is not None else got.keys()):
        g, w = got[k], want[k]
        if k == 'selected':
            assert len(g) == len(w), k
            for t, (a, b) in enumerate(zip(g, w)):
                assert a.dtype == b.dtype and np.array_equal(a, b), '%s[%d]' % (k, t)
        else:
            assert g.dtype == w.dtype and np.array_equal(g, w), k


def dense(rows, cols, n_rows, n_cols):
    X = np.zeros((int(n_rows), int(n_cols)), dtype=bool)
    X[np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)] = True
    return X


class ModelContext(object):
    """Stands in for _native.Context where only the host side is under test: core_select() and row_counts() with the
    binding's arguments and result layout, computed by the model."""
    calls = 0

    def core_select(self, allele_rows, allele_genomes, n_alleles, n_genomes, run_start, thresholds, gene_rows=None,
                    gene_genomes=None, n_genes=0, gene_of_run=None, want=OUTPUTS):
        self.calls += 1
        thresholds = np.asarray(thresholds, dtype=np.uint32)
        assert 1 <= thresholds.size <= 32
        pairs = np.asarray(allele_rows, dtype=np.int64) * int(n_genomes) + np.asarray(allele_genomes, dtype=np.int64)
        dups = [pairs.size - np.unique(pairs).size, 0]
        G = None
        if gene_of_run is not None:
            gene_rows = [] if gene_rows is None else gene_rows
            gene_genomes = [] if gene_genomes is None else gene_genomes
            pairs = np.asarray(gene_rows, dtype=np.int64) * int(n_genomes) + np.asarray(gene_genomes, dtype=np.int64)
            dups[1] = pairs.size - np.unique(pairs).size
            G = dense(gene_rows, gene_genomes, n_genes, n_genomes)
        if any(dups):
            return None, tuple(dups)
        out = select(dense(allele_rows, allele_genomes, n_alleles, n_genomes), run_start, thresholds, G, gene_of_run)
        return {k: out[k] for k in OUTPUTS if k in set(want) | ({'n_selected'} if 'selected' in want else set())}, (0, 0)

    def row_counts(self, rows, cols, n_rows, n_cols):
        X = dense(rows, cols, n_rows, n_cols)
        return X.sum(axis=1).astype(np.int32), int(np.asarray(rows).size - X.sum())


# -- fixtures (tests/golden/core_fasta, written by tests/golden/make_golden_core_fasta.py) --------------------------------
def _hand(name, d):
    base = os.path.join(GOLDEN, d, name)
    return {'allele_npz': base + '_strain_by_allele.npz', 'allele_labels': base + '_strain_by_allele.npz.labels.txt',
            'gene_npz': base + '_strain_by_gene.npz', 'gene_labels': base + '_strain_by_gene.npz.labels.txt',
            'faa': base + '_nr.faa'}


INPUTS = {'cds': {'allele_npz': os.path.join(CDS, 'T_strain_by_allele.npz'),
                  'allele_labels': os.path.join(CDS, 'T_strain_by_allele.npz.labels.txt'),
                  'gene_npz': os.path.join(CDS, 'T_strain_by_gene.npz'),
                  'gene_labels': os.path.join(CDS, 'T_strain_by_gene.npz.labels.txt'), 'faa': os.path.join(CDS, 'T_nr.faa')},
          'hand': _hand('H', 'hand_in'), 'name_a': _hand('PAO1', 'name_a_in')}
# case -> (inputs, genomes_num); None: create_alleles_fasta
CORE_CASES = {'cds_core_1': ('cds', 1), 'cds_core_3': ('cds', 3), 'cds_core_7': ('cds', 7), 'hand_core_1': ('hand', 1),
              'hand_core_3': ('hand', 3), 'hand_core_5': ('hand', 5), 'hand_core_6': ('hand', 6), 'name_a_core_2': ('name_a', 2)}
ALLELE_CASES = {'cds_alleles': 'cds', 'hand_alleles': 'hand', 'name_a_alleles': 'name_a'}


def load_case(case):
    with open(os.path.join(GOLDEN, case, 'result.json')) as f:
        result = json.load(f)
    path = os.path.join(GOLDEN, case, 'out.faa')
    result['out_faa'] = open(path, 'rb').read() if os.path.exists(path) else None
    return result


def to_pandas(rec):
    """The frame or Series a fixture recorded."""
    import pandas as pd
    if rec['kind'] == 'series':
        return pd.Series(rec['values'], index=pd.Index(rec['index'], dtype=rec['index_dtype']), name=rec['name'],
                         dtype=rec['dtype'])
    if not rec['columns']:
        return pd.DataFrame([])
    cols = {}
    for j, (c, t) in enumerate(zip(rec['columns'], rec['dtypes'])):
        cols[c] = pd.Series([row[j] for row in rec['values']], dtype=t)
    df = pd.DataFrame(cols, columns=rec['columns'])
    if rec['index_class'] != 'RangeIndex':
        df.index = pd.Index(rec['index'], dtype=rec['index_dtype'])
    return df


def assert_same_pandas(got, rec):
    """got equals what the reference returned: values, columns, dtypes, index and the index's class."""
    import pandas as pd
    want = to_pandas(rec)
    if rec['kind'] == 'series':
        pd.testing.assert_series_equal(got, want, check_index_type='equiv')
        return
    pd.testing.assert_frame_equal(got, want, check_index_type='equiv', check_column_type='equiv')
    assert [str(t) for t in got.dtypes] == rec['dtypes']
    assert type(got.index).__name__ == rec['index_class']
    assert [type(c).__name__ for c in got.columns] == ['str'] * len(rec['columns'])


def tables(inputs):
    """(A, G, allele labels, gene labels) of a fixture's inputs as dense bool tables and lists of row labels."""
    files = INPUTS[inputs] if isinstance(inputs, str) else inputs          # (or a dict of paths like those of INPUTS)
    out = []
    for k in ('allele', 'gene'):
        z = np.load(files[k + '_npz'])
        shape = tuple(int(x) for x in z['shape'])
        out.append(dense(z['row'], z['col'], *shape))
    labels = []
    for k, X in zip(('allele', 'gene'), out):
        with open(files[k + '_labels']) as f:
            labels.append(f.read().split('\n')[:X.shape[0]])
    return out[0], out[1], labels[0], labels[1]


def reference_selection(inputs, thresholds, with_gene_table=True):
    """The model's `selected` allele names per threshold, by the grouping of validate_gene_table restated with loops in
    allele_runs_model.runs_by_name (gene name = the label up to its last `A`)."""
    A, G, allele_labels, gene_labels = tables(inputs)
    _, run_start, gene_of_run, order = allele_runs_model.runs_by_name(gene_labels, allele_labels)
    out = select(A[order], run_start, thresholds, G if with_gene_table else None, gene_of_run)
    return [[allele_labels[order[i]] for i in sel] for sel in out['selected']]

