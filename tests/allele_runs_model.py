"""TEST INFRASTRUCTURE: a plain-numpy restatement (one thread) of the outputs of pgx_allele_runs (include/pgx.h, "Runs of
allele rows"; pangenomix_amd/csrc/runs.hip) from DENSE 0/1 tables, plus the helpers the tests share: bit
packing in the library's layout and the reader of tests/golden/consistency. tests/test_consistency_host.py checks the model
against the counts the reference printed for every fixture, so it is a fair yardstick for the sizes no fixture covers.

    derived[r, j]   = any(A[run_start[r]:run_start[r + 1], j])
    diff[r, j]      = derived[r, j] != (G[gene_of_run[r], j] if gene_of_run[r] >= 0 else 0)
    total[r]        = sum of the row counts of the run
    best_allele[r]  = first row of the run with the largest count (-1 for an empty run), best_count[r] that count
"""
import os
import re

import numpy as np


def stride_words(n_rows):
    """pgx_bitmap_stride_words: 64-bit words per genome, rows padded to a multiple of 16 words, at least 16."""
    return max(16, ((int(n_rows) + 63) // 64 + 15) // 16 * 16)


def pack(X):
    """uint64 [n_genomes, stride_words(n_rows)] of the bool table X [n_rows, n_genomes]: row r is bit r % 64 of word r // 64."""
    X = np.asarray(X, dtype=bool)
    n_rows, n_genomes = X.shape
    stride = stride_words(n_rows)
    padded = np.zeros((n_genomes, stride * 64), dtype=np.uint8)
    padded[:, :n_rows] = X.T
    return np.packbits(padded, axis=1, bitorder='little').view('<u8').reshape(n_genomes, stride).astype(np.uint64)


def unpack(bits, n_rows):
    """bool [n_rows, n_genomes] of a bitmap in the library's layout (pad bits dropped)."""
    bits = np.ascontiguousarray(bits, dtype='<u8')
    return np.unpackbits(bits.view(np.uint8), axis=1, bitorder='little')[:, :int(n_rows)].T.astype(bool)


def pad_bits_clear(bits, n_rows):
    """True iff every bit of the bitmap at or beyond row n_rows is 0."""
    bits = np.ascontiguousarray(bits, dtype='<u8')
    return not np.unpackbits(bits.view(np.uint8), axis=1, bitorder='little')[:, int(n_rows):].any()


def runs(A, run_start, G=None, gene_of_run=None):
    """dict of the seven outputs (the bitmaps as bool [n_runs, n_genomes]) from the bool tables A [n_alleles, n_genomes]
    and G [n_genes, n_genomes]."""
    A = np.asarray(A, dtype=bool)
    run_start = np.asarray(run_start, dtype=np.int64)
    n_runs, n_genomes = run_start.size - 1, A.shape[1]
    counts = A.sum(axis=1, dtype=np.int64)
    derived = np.zeros((n_runs, n_genomes), dtype=bool)
    gene = np.zeros((n_runs, n_genomes), dtype=bool)
    total = np.zeros(n_runs, dtype=np.uint64)
    best_allele = np.full(n_runs, -1, dtype=np.int32)
    best_count = np.zeros(n_runs, dtype=np.uint32)
    for r in range(n_runs):
        a, b = int(run_start[r]), int(run_start[r + 1])
        if b > a:
            derived[r] = A[a:b].any(axis=0)
            total[r] = counts[a:b].sum()
            best_allele[r] = a + int(np.argmax(counts[a:b]))          # (argmax: the first of equal maxima)
            best_count[r] = counts[best_allele[r]]
        if G is not None and gene_of_run is not None and int(gene_of_run[r]) >= 0:
            gene[r] = np.asarray(G, dtype=bool)[int(gene_of_run[r])]
    diff = derived != gene
    return {'derived': derived, 'diff': diff, 'diff_per_genome': diff.sum(axis=0).astype(np.uint32),
            'diff_per_run': diff.sum(axis=1).astype(np.uint32), 'total': total, 'best_allele': best_allele,
            'best_count': best_count}


def assert_equal(got, want, n_runs):
    """Exact equality of a result dict of Context.allele_runs (bitmaps packed) with the model's; pad bits of the bitmaps 0."""
    for k, w in want.items():
        g = got[k]
        if k in ('derived', 'diff'):
            assert g.shape == (w.shape[1], stride_words(n_runs)), k
            assert pad_bits_clear(g, n_runs), k + ': pad bits set'
            g = unpack(g, n_runs)
        assert g.dtype == w.dtype and np.array_equal(g, w), k


# -- the run construction of the two grouping rules, restated with plain loops ------------------------------------------
def gene_of(allele):
    return allele[:allele.rindex('A')] if 'A' in allele else ''


def runs_by_name(gene_labels, allele_labels):
    """validate_gene_table's grouping: one run per gene row, then one per gene name that occurs only among the alleles (in
    order of first appearance). Returns (run names, run_start, gene_of_run, order) where order[k] = the allele row that is
    row k of the gene-sorted table."""
    names = list(gene_labels)
    pos = {g: i for i, g in enumerate(names)}
    members = [[] for _ in names]
    for i, a in enumerate(allele_labels):
        g = gene_of(a)
        if g not in pos:
            pos[g] = len(names)
            names.append(g)
            members.append([])
        members[pos[g]].append(i)
    run_start = np.cumsum([0] + [len(m) for m in members])
    gene_of_run = np.array([i if i < len(gene_labels) else -1 for i in range(len(names))], dtype=np.int32)
    return names, run_start, gene_of_run, np.array([i for m in members for i in m], dtype=np.int64)


def runs_in_order(allele_labels, name_of=gene_of):
    """The table-order grouping: maximal stretches of consecutive allele rows with one gene name. (names, run_start)."""
    names, starts = [], []
    for i, a in enumerate(allele_labels):
        g = name_of(a)
        if not names or names[-1] != g:
            names.append(g)
            starts.append(i)
    return names, np.array(starts + [len(allele_labels)], dtype=np.int64)


# -- fixtures (tests/golden/consistency/*.npz, written by tests/golden/make_golden_consistency.py) -------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'consistency')


def load_case(path):
    """dict of a fixture: 'genes' / 'alleles' = (values float64 [n_rows, n_genomes] with NaN for absent, index, columns),
    the recorded stdout of the two validators, df_dominant's columns, the two FASTA texts."""
    d = np.load(path)
    out = {}
    for t in ('genes', 'alleles'):
        shape = tuple(int(x) for x in d[t + '_shape'])
        values = np.full(shape, np.nan)
        values[d[t + '_rows'].astype(np.int64), d[t + '_cols'].astype(np.int64)] = d[t + '_values']
        out[t] = (values, [str(x) for x in d[t + '_index']], [str(x) for x in d[t + '_columns']])
    for k in ('stdout_validate', 'stdout_dense', 'faa', 'dominant_faa'):
        out[k] = bytes(d[k]).decode('utf-8')
    out['dense_raises'] = str(d['dense_raises'])
    out['dominant'] = {k: d['dominant_' + k] for k in ('gene', 'dominant_allele', 'gene_count', 'allele_count')}
    out['dominant']['gene'] = [str(x) for x in out['dominant']['gene']]
    out['dominant']['dominant_allele'] = [str(x) for x in out['dominant']['dominant_allele']]
    return out


def frames(case):
    """(df_genes, df_alleles): the pandas frames the reference was run on."""
    import pandas as pd
    return tuple(pd.DataFrame(v, index=i, columns=c) for v, i, c in (case['genes'], case['alleles']))


def expected_dominant(case):
    import pandas as pd
    d = case['dominant']
    df = pd.DataFrame({'gene': d['gene'], 'dominant_allele': d['dominant_allele'],
                       'gene_count': np.asarray(d['gene_count'], dtype=np.float64),
                       'allele_count': np.asarray(d['allele_count'], dtype=np.float64)})
    return df.set_index('gene')


_SET = re.compile(r"^\tInconsistent: \{(.*)\}$")


def parse_validate_stdout(text):
    """validate_gene_table's output as (lines with every `Inconsistent:` set replaced by a frozenset of its names, count):
    the order in which a set prints its elements is not part of the contract."""
    lines, count = [], None
    for line in text.splitlines():
        m = _SET.match(line)
        if m:
            lines.append(frozenset(re.findall(r"'([^']*)'", m.group(1))))
        else:
            lines.append(line)
            if line.startswith('Gene Table Inconsistencies: '):
                count = int(line.rsplit(' ', 1)[1])
    return lines, count


def parse_dense_stdout(text):
    """validate_gene_table_dense's output as (lines, count, names printed after `Inconsistent`)."""
    lines = text.splitlines()
    count = [int(x.rsplit(' ', 1)[1]) for x in lines if x.startswith('Gene Table Inconsistencies: ')]
    return lines, (count[0] if count else None), [x.split(' ', 1)[1] for x in lines if x.startswith('Inconsistent ')]


class ModelContext(object):
    """Stands in for _native.Context where only the host side is under test: allele_runs() with the binding's arguments and
    result layout, computed by runs() above."""

    def allele_runs(self, allele_rows, allele_genomes, n_alleles, n_genomes, run_start, gene_rows=None, gene_genomes=None,
                    n_genes=0, gene_of_run=None, want=()):
        A = np.zeros((int(n_alleles), int(n_genomes)), dtype=bool)
        A[np.asarray(allele_rows, dtype=np.int64), np.asarray(allele_genomes, dtype=np.int64)] = True
        G = None
        if gene_of_run is not None:
            G = np.zeros((int(n_genes), int(n_genomes)), dtype=bool)
            G[np.asarray(gene_rows, dtype=np.int64), np.asarray(gene_genomes, dtype=np.int64)] = True
        out = runs(A, run_start, G, gene_of_run)
        for k in ('derived', 'diff'):
            out[k] = pack(out[k])
        return {k: out[k] for k in want}, (0, 0)


def lsdf_pair(case, keep_zeros=False):
    """The fixture's two tables as LightSparseDataFrames: a cell is stored (as 1) iff the frame's value is 1, which is the
    same table to the functions that read NaN and 0 as absent. keep_zeros: a 0.0 of the frame is stored as a zero."""
    import scipy.sparse
    from pangenomix_amd import sparse_utils
    out = []
    for values, index, columns in (case['genes'], case['alleles']):
        r, c = np.nonzero(~np.isnan(values) if keep_zeros else values == 1)
        coo = scipy.sparse.coo_matrix((values[r, c].astype(np.int64), (r, c)), shape=values.shape)
        out.append(sparse_utils.LightSparseDataFrame(np.array(index), np.array(columns), coo))
    return tuple(out)


def has_stored_zero(case):
    return any(bool(np.any(case[t][0] == 0)) for t in ('genes', 'alleles'))


def check_python_functions(case, ctx, tmp_dir, as_lsdf):
    """The three functions of pangenomix_amd.pangenome on one fixture against what the reference printed, returned and
    wrote: counts and df_dominant equal, the FASTA byte-equal, stdout line-equal (the `Inconsistent:` sets as sets).
    as_lsdf: the same tables as LightSparseDataFrames. What dropna() makes of a 0.0 cell has no LSDF counterpart: a stored
    zero is refused (the rule of sparse_utils._screen_table), so on a fixture with such a cell validate_gene_table's LSDF
    run has to raise ValueError instead of printing the recording."""
    import contextlib
    import io

    import pandas as pd
    from pangenomix_amd import pangenome

    def captured(fn, *args):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            value = fn(*args, ctx=ctx)
        return value, buf.getvalue()

    dfg, dfa = lsdf_pair(case) if as_lsdf else frames(case)
    if as_lsdf and has_stored_zero(case):
        try:
            captured(pangenome.validate_gene_table, *lsdf_pair(case, keep_zeros=True))
        except ValueError as e:
            assert 'stored zeros' in str(e)
        else:
            raise AssertionError('validate_gene_table took an LSDF with a stored zero')
    else:
        n, text = captured(pangenome.validate_gene_table, dfg, dfa, 1)
        want_lines, want_n = parse_validate_stdout(case['stdout_validate'])
        assert n == want_n
        assert parse_validate_stdout(text)[0] == want_lines
    if case['dense_raises']:
        assert case['dense_raises'] == 'KeyError'
        try:
            captured(pangenome.validate_gene_table_dense, dfg, dfa)
        except KeyError:
            pass
        else:
            raise AssertionError('validate_gene_table_dense did not raise KeyError')
    else:
        n, text = captured(pangenome.validate_gene_table_dense, dfg, dfa)
        want_lines, want_n, _ = parse_dense_stdout(case['stdout_dense'])
        assert n == want_n
        assert text.splitlines() == want_lines
    faa, dom = os.path.join(tmp_dir, 'alleles.faa'), os.path.join(tmp_dir, 'dominant.faa')
    with open(faa, 'w') as f:
        f.write(case['faa'])
    df, _ = captured(pangenome.extract_dominant_alleles, dfa, faa, dom)
    pd.testing.assert_frame_equal(df, expected_dominant(case))
    with open(dom, 'rb') as f:
        assert f.read() == case['dominant_faa'].encode('utf-8')
