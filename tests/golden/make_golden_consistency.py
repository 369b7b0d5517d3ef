#!/usr/bin/env python
"""Golden fixtures for the gene-table / allele-table consistency checks and the dominant-allele extraction (reference
pangenome.py validate_gene_table :1246-1277, validate_gene_table_dense :1280-1330, extract_dominant_alleles :1812-1889),
produced by RUNNING THE REFERENCE on the CPU in the build container (needs /root/reference; it never travels to the GPU
box):

    python tests/golden/make_golden_consistency.py

Only data is written. tests/golden/consistency/<case>.npz holds
  genes_* / alleles_*   the two pandas frames the reference was given (float64, NaN = absent): shape, index, columns and
                        the cells that are not NaN as rows / cols / values (a stored 0.0 is such a cell)
  stdout_validate       what validate_gene_table printed (utf-8 bytes)
  stdout_dense          what validate_gene_table_dense printed; dense_raises = the name of the exception it raised
                        instead ('' = none): a run whose gene is missing from the gene table is a KeyError from .loc
  dominant_*            the columns of the returned df_dominant (index `gene`); the counts are float64 there
  faa, dominant_faa     the allele FASTA handed to extract_dominant_alleles and the bytes it wrote
"""
import contextlib
import io
import os
import sys
import tempfile

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, '/root/reference')

import pangenomix.pangenome as ref      # noqa: E402

OUT = os.path.join(HERE, 'consistency')
GENOMES = ['g%d' % j for j in range(6)]


def tables(rng, clusters, alleles_per=(1, 2, 3), density=0.45):
    """(df_genes, df_alleles) for the given cluster numbers: every allele row random, the gene row the OR of its alleles;
    rows in the order of the names sorted as strings, as the pipeline writes them."""
    allele_rows = {}
    for k, c in enumerate(clusters):
        for m in range(alleles_per[k % len(alleles_per)]):
            allele_rows['Test_C%dA%d' % (c, m)] = rng.random(len(GENOMES)) < density
    names = sorted(allele_rows)
    A = np.array([allele_rows[n] for n in names])
    genes = sorted({n[:n.rindex('A')] for n in names})
    G = np.array([np.any([allele_rows[n] for n in names if n[:n.rindex('A')] == g], axis=0) for g in genes])
    as_frame = lambda X, idx: pd.DataFrame(np.where(X, 1.0, np.nan), index=idx, columns=GENOMES)   # noqa: E731
    return as_frame(G, genes), as_frame(A, names)


def fasta_for(alleles, rng, extra=('Test_C999A0',)):
    """An allele FASTA: every allele (and a name that is in no table), sequences of one to three lines."""
    out = []
    for name in list(alleles) + list(extra):
        out.append('>' + name + '\n')
        for _ in range(int(rng.integers(1, 4))):
            out.append(''.join(rng.choice(list('ACDEFGHIKLMNPQRSTVWY'), int(rng.integers(5, 30)))) + '\n')
    return ''.join(out)


def cells(df, prefix):
    values = df.values.astype(np.float64)
    rows, cols = np.nonzero(~np.isnan(values))
    return {prefix + '_shape': np.array(values.shape, dtype=np.int64), prefix + '_index': np.array(df.index.tolist()),
            prefix + '_columns': np.array(df.columns.tolist()), prefix + '_rows': rows.astype(np.uint16),
            prefix + '_cols': cols.astype(np.uint16), prefix + '_values': values[rows, cols]}


def record(name, dfg, dfa, rng):
    out = {}
    out.update(cells(dfg, 'genes'))
    out.update(cells(dfa, 'alleles'))
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        ref.validate_gene_table(dfg, dfa)
    out['stdout_validate'] = np.frombuffer(buf.getvalue().encode('utf-8'), dtype=np.uint8)
    buf, raised = io.StringIO(), ''
    try:
        with contextlib.redirect_stdout(buf):
            ref.validate_gene_table_dense(dfg, dfa)
    except Exception as e:                  # noqa: BLE001 (recorded: what the port has to raise as well)
        raised = type(e).__name__
    out['stdout_dense'] = np.frombuffer(buf.getvalue().encode('utf-8'), dtype=np.uint8)
    out['dense_raises'] = np.array(raised)
    faa = fasta_for(dfa.index, rng)
    with tempfile.TemporaryDirectory() as tmp:
        faa_path, dom_path = os.path.join(tmp, 'alleles.faa'), os.path.join(tmp, 'dominant.faa')
        with open(faa_path, 'w') as f:
            f.write(faa)
        with contextlib.redirect_stdout(io.StringIO()):
            dom = ref.extract_dominant_alleles(dfa, faa_path, dom_path)
        with open(dom_path, 'rb') as f:
            out['dominant_faa'] = np.frombuffer(f.read(), dtype=np.uint8)
    out['faa'] = np.frombuffer(faa.encode('utf-8'), dtype=np.uint8)
    assert dom.index.name == 'gene' and list(dom.columns) == ['dominant_allele', 'gene_count', 'allele_count']
    assert dom.gene_count.dtype == np.float64 and dom.allele_count.dtype == np.float64
    out['dominant_gene'] = np.array(dom.index.tolist(), dtype='U')
    out['dominant_dominant_allele'] = np.array(dom.dominant_allele.tolist(), dtype='U')
    out['dominant_gene_count'] = dom.gene_count.values
    out['dominant_allele_count'] = dom.allele_count.values
    path = os.path.join(OUT, name + '.npz')
    np.savez_compressed(path, **out)
    count = [x for x in bytes(out['stdout_validate']).decode().splitlines() if x.startswith('Gene Table')]
    print('%-24s genes %s alleles %s | %s | dense: %s | dominant %d | %d bytes'
          % (name, dfg.shape, dfa.shape, count[0], raised or bytes(out['stdout_dense']).decode().splitlines()[-1],
             len(dom), os.path.getsize(path)))


def main():
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(61)
    dfg, dfa = tables(rng, range(6))
    record('consistent', dfg, dfa, rng)

    dfg, dfa = tables(rng, range(6))
    absent = np.argwhere(np.isnan(dfg.values))[0]
    present = np.argwhere(~np.isnan(dfg.values))[-1]
    dfg.iloc[absent[0], absent[1]] = 1.0
    dfg.iloc[present[0], present[1]] = np.nan
    record('flipped_gene_cells', dfg, dfa, rng)

    dfg, dfa = tables(rng, range(5))
    dfg.loc['Test_C7'] = [1.0, np.nan, np.nan, 1.0, np.nan, np.nan]      # a gene row that no allele stands for
    dfg.loc['Test_C8'] = np.nan                                          # ... and one that is empty as well
    record('gene_without_alleles', dfg, dfa, rng)

    dfg, dfa = tables(rng, range(5))
    dfa.loc['Test_C9A0'] = [np.nan, 1.0, 1.0, np.nan, np.nan, 1.0]        # its gene Test_C9 is not in the gene table
    record('allele_gene_missing', dfg, dfa, rng)

    dfg, dfa = tables(rng, range(5))
    r, c = np.argwhere(np.isnan(dfg.values))[2]
    first = [i for i, n in enumerate(dfa.index) if n.startswith(dfg.index[r] + 'A')][0]
    dfa.iloc[first, c] = 0.0          # a stored zero: present to dropna(), absent to fillna(0)
    r0, c0 = np.argwhere(np.isnan(dfg.values))[0]
    dfg.iloc[r0, c0] = 0.0            # ... and one in the gene table
    record('explicit_zero', dfg, dfa, rng)

    dfg, dfa = tables(rng, range(4), alleles_per=(3,))
    dfa.loc['Test_C1A0'] = [1.0, 1.0, np.nan, np.nan, np.nan, np.nan]
    dfa.loc['Test_C1A1'] = [np.nan, np.nan, 1.0, 1.0, 1.0, np.nan]       # the largest count, twice: the first wins
    dfa.loc['Test_C1A2'] = [1.0, np.nan, 1.0, np.nan, np.nan, 1.0]
    dfg.loc['Test_C1'] = [1.0, 1.0, 1.0, 1.0, 1.0, 1.0]
    record('count_tie', dfg, dfa, rng)

    dfg, dfa = tables(rng, range(5))
    for n in dfa.index:
        if n.startswith('Test_C2A'):
            dfa.loc[n] = np.nan
    dfg.loc['Test_C2'] = np.nan
    record('all_absent_gene', dfg, dfa, rng)

    dfg, dfa = tables(rng, range(4), alleles_per=(2, 3))
    order = list(dfa.index)
    moved = [n for n in order if n.startswith('Test_C1A')][-1]           # the last allele of C1 goes behind C2's
    order.remove(moved)
    order.insert(max(i for i, n in enumerate(order) if n.startswith('Test_C2A')) + 1, moved)
    record('recurring_gene', dfg, dfa.loc[order], rng)

    dfg, dfa = tables(rng, (1, 2, 10, 100))
    assert list(dfg.index) == ['Test_C1', 'Test_C10', 'Test_C100', 'Test_C2']
    dfg.iloc[1, 0] = np.nan if dfg.iloc[1, 0] == 1.0 else 1.0
    record('lexicographic_clusters', dfg, dfa, rng)


if __name__ == '__main__':
    main()
