"""The reference's core_genome module on MI355X, complete: how many genomes hold each gene or allele, which
genes are core, which allele of each gene is the most common, and the FASTA file of those alleles
(create_core_genes_fasta, the README's "Core and accessory genome" workflow). Same arguments, same DataFrames, same
printed lines as reference core_genome.py:7-219.
  * The counts are row popcounts of the device bitmap (libpgx, csrc/pancore.hip).
  * create_core_genes_fasta / core_allele_sets make ONE library call (csrc/select.hip, pgx_core_select): gene counts, the
    dominant allele of every gene and the ordered list of selected alleles for up to 32 thresholds at once; then one pass
    over the input FASTA file serves every threshold. No per-gene Python object is built.
  * The frame-in / frame-out helpers (identify_gene_allele_rows, subset_genes_alleles_pairs,
    find_highest_allele_expression, find_allele_names) are vectorised host code that returns the reference's frames quirk
    for quirk -- they exist for callers that chain them by hand.
  * filter_sequences is host I/O. Biopython (the reference's reader and writer) is replaced by the rules in its docstring.
Where this differs from the reference, on inputs on which the reference fails or reads shifted rows: INTEGRATION.md."""
from __future__ import print_function

import ast
import math

import numpy as np
import pandas as pd

from . import _native

# what pandas' CSV reader turns into NaN (read_csv, default na_values): the reference reads its label files with it
_NA_SPELLINGS = frozenset(['', '#N/A', '#N/A N/A', '#NA', '-1.#IND', '-1.#QNAN', '-NaN', '-nan', '1.#IND', '1.#QNAN', '<NA>',
                           'N/A', 'NA', 'NULL', 'NaN', 'None', 'n/a', 'nan', 'null'])
_MAX_THRESHOLDS = 32               # csrc/select.hip


def _row_occurrence(npz_file, index_name, ctx=None):
    """[index_name int32, count int64] for every row with at least one entry, ascending."""
    with np.load(npz_file) as data:
        rows, cols = data['row'], data['col']
        shape = tuple(int(x) for x in data['shape']) if 'shape' in data.files else None
    n_rows = shape[0] if shape else (int(rows.max()) + 1 if rows.size else 0)
    n_cols = shape[1] if shape else (int(cols.max()) + 1 if cols.size else 0)
    ctx = ctx or _native.default_context()
    counts, dup = ctx.row_counts(rows, cols, n_rows, n_cols)
    if dup:   # the reference counts triples, duplicates included; the bitmap counts genomes
        counts = np.bincount(rows, minlength=n_rows).astype(np.int32)
    present = np.flatnonzero(counts > 0)
    return pd.DataFrame({index_name: present.astype(rows.dtype), 'count': counts[present].astype(np.int64)})


def count_gene_occurence(gene_npz_file, ctx=None):
    """Occurrence of each gene over all genomes (reference core_genome.py:127-155)."""
    df = _row_occurrence(gene_npz_file, 'gene_index', ctx)
    print("\nCounted gene occurence")
    return df


def count_allele_occurence(allele_npz_file, ctx=None):
    """Occurrence of each allele over all genomes (reference core_genome.py:191-219)."""
    df = _row_occurrence(allele_npz_file, 'allele_index', ctx)
    print("\nCounted allele occurence")
    return df


def find_core_genes(gene_occurrence_count, genomes_num):
    """Genes present in at least `genomes_num` genomes (reference core_genome.py:107-124: columns
    gene_index / highest_expression; an empty frame without columns when there is none)."""
    hit = gene_occurrence_count[gene_occurrence_count['count'] >= genomes_num]
    if hit.empty:
        return pd.DataFrame([])
    return pd.DataFrame({'gene_index': hit['gene_index'].values.astype(np.int64),
                         'highest_expression': hit['count'].values.astype(np.int64)})


# ---------------------------------------------------------------------------
# label files
# ---------------------------------------------------------------------------
def _read_labels(label_file):
    """The lines of a label file (row labels, then genome labels), as the reference's pd.read_csv(header=None) gives them.
    A line that reader would alter, split or drop -- a comma, a double quote, blanks at either end, a spelling of NA, an
    empty line -- raises ValueError naming it: every row behind it would silently get another label."""
    with open(label_file) as f:
        lines = f.read().split('\n')
    if lines and lines[-1] == '':
        lines.pop()
    for i, line in enumerate(lines):
        if line.endswith('\r'):
            line = lines[i] = line[:-1]
        if ',' in line or '"' in line or line != line.strip() or line in _NA_SPELLINGS:
            raise ValueError('%s, line %d: the label %r is not read back as it stands by a CSV reader'
                             % (label_file, i + 1, line))
    return lines


def _labels_frame(label_file, column):
    return pd.DataFrame({column: pd.Series(_read_labels(label_file), dtype=object)})


def identify_gene_allele_rows(gene_npz_label_file, allele_npz_label_file):
    """The allele rows of every gene (reference core_genome.py:157-187 = :222-252): columns gene (int64) and allele_index
    (a list of ints per gene), one row per gene that has an allele, ascending. The reference's quirks are kept: both
    files are read WHOLE, so the genome labels behind the row labels are "alleles" and "genes" too (a genome label
    without an `A` pairs with itself); an allele's gene name is the first maximal run of characters other than `A`."""
    gene_df = _labels_frame(gene_npz_label_file, 'gene_name')
    allele_df = _labels_frame(allele_npz_label_file, 'allele_name')
    gene_df['gene'] = gene_df.index
    allele_df['gene_name'] = allele_df['allele_name'].str.extract(r'([^A]+)')
    merged = pd.merge(allele_df, gene_df, on='gene_name', how='left')
    gene = merged['gene'].values.astype(np.float64)
    rows = np.flatnonzero(~np.isnan(gene))
    rows = rows[np.argsort(gene[rows], kind='stable')]
    genes, first = np.unique(gene[rows], return_index=True)
    lists = [part.tolist() for part in np.split(rows, first[1:])] if rows.size else []
    result = pd.DataFrame({'gene': genes.astype(np.int64), 'allele_index': pd.Series(lists, dtype=object)},
                          columns=['gene', 'allele_index'])
    print("\nIdentified all alleles per genome")
    return result


def subset_genes_alleles_pairs(allele_occurence_count, highest_gene_expression_rows):
    """The rows of identify_gene_allele_rows' frame whose gene is among find_core_genes' (reference :97-104); KeyError
    ('gene_index') when find_core_genes found none, as in the reference."""
    target_genes = highest_gene_expression_rows['gene_index'].unique()
    return allele_occurence_count[allele_occurence_count['gene'].isin(target_genes)].copy()


def _highest_expression(row_counts_df, gene_allele_rows_df):
    """One row per row of gene_allele_rows_df: gene, and the label of the first of its allele_index entries with the
    largest `count` in row_counts_df (looked up BY LABEL, as .loc does). allele_index: lists, or their string form."""
    if len(gene_allele_rows_df) == 0:
        return pd.DataFrame([])
    lists = [x if isinstance(x, list) else ast.literal_eval(x) for x in gene_allele_rows_df['allele_index'].tolist()]
    lengths = np.fromiter((len(x) for x in lists), dtype=np.int64, count=len(lists))
    if (lengths == 0).any():
        raise ValueError('attempt to get argmax of an empty sequence')
    flat = np.concatenate([np.asarray(x, dtype=np.int64) for x in lists])
    at = row_counts_df.index.get_indexer(flat)
    if (at < 0).any():
        raise KeyError('%r not in index' % flat[at < 0].tolist())
    counts = row_counts_df['count'].values[at]
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    top = np.maximum.reduceat(counts, starts)
    is_top = np.flatnonzero(counts == np.repeat(top, lengths))
    run_of = np.repeat(np.arange(lengths.size), lengths)[is_top]
    first = is_top[np.concatenate([[True], run_of[1:] != run_of[:-1]])]
    return pd.DataFrame({'gene': gene_allele_rows_df['gene'].values.astype(np.int64),
                         'highest_expression': flat[first]}, columns=['gene', 'highest_expression'])


def find_highest_allele_expression(row_counts_df, gene_allele_rows_df):
    """The most common allele of every gene (reference :66-95): columns gene / highest_expression (int64), the first
    allele winning a tie; an empty frame without columns for no genes."""
    return _highest_expression(row_counts_df, gene_allele_rows_df)


def find_allele_names(highest_expression_rows, allele_npz_label_file):
    """The names of the rows in column highest_expression (reference :48-62): a Series `allele_name` on the frame's index.
    As in the reference the frame's `gene` column is cast to int IN PLACE."""
    allele_labels_df = _labels_frame(allele_npz_label_file, 'allele_name')
    highest_expression_rows['gene'] = highest_expression_rows['gene'].astype(int)
    names = pd.merge(highest_expression_rows, allele_labels_df, left_on='highest_expression', right_index=True)
    print("\nFound the alleles with the highest expression per gene")
    return names['allele_name']


# ---------------------------------------------------------------------------
# FASTA
# ---------------------------------------------------------------------------
def _filter_fasta(input_faa, name_lists, output_files):
    """One pass over input_faa for all (names, output file) pairs; the rules of filter_sequences."""
    member = {}
    for t, names in enumerate(name_lists):
        bit = 1 << t
        for name in (names.tolist() if hasattr(names, 'tolist') else list(names)):
            member[name] = member.get(name, 0) | bit
    outs = []
    try:
        with open(input_faa) as f:
            for path in output_files:
                outs.append(open(path, 'w'))
            mask, parts = 0, []

            def flush():
                if mask:
                    seq = ''.join(parts)
                    body = ''.join([seq[i:i + 60] + '\n' for i in range(0, len(seq), 60)])
                    for t, out in enumerate(outs):
                        if (mask >> t) & 1:
                            out.write(body)

            for line in f:
                if line[:1] == '>':
                    flush()
                    title = line[1:].rstrip()
                    words = title.split(None, 1)
                    mask = member.get((words[0] if words else '').split('|')[0], 0)
                    parts = []
                    if mask:
                        for t, out in enumerate(outs):
                            if (mask >> t) & 1:
                                out.write('>' + title + '\n')
                elif mask:
                    parts.append(''.join(line.split()))
            flush()
    finally:
        for out in outs:
            out.close()


def filter_sequences(input_faa, highest_expression_names, output_faa):
    """Writes the records of input_faa whose allele name is among highest_expression_names to output_faa (reference
    :28-44). The input is streamed; host only. The reference reads and writes through Biopython, which is replaced by
    these rules, restated from its FASTA reader and writer:
      * a record starts at a line beginning with `>`; its title is the rest of that line, right-stripped; its id is the
        first whitespace-separated word of the title; lines before the first record are skipped;
      * a record is kept iff id.split('|')[0] is among the names;
      * a kept record is written as `>` + title, then its sequence with all blanks removed, re-wrapped at 60 columns
        (an empty sequence writes no line);
      * output follows input-file order, and a record given twice is written twice."""
    print("\nCreated a FASTA file with all the highly expressed alleles. Success!")
    _filter_fasta(input_faa, [highest_expression_names], [output_faa])


# ---------------------------------------------------------------------------
# the two workflows, through one library call
# ---------------------------------------------------------------------------
def _load_coo(npz_file):
    with np.load(npz_file) as data:
        rows, cols = data['row'], data['col']
        shape = tuple(int(x) for x in data['shape']) if 'shape' in data.files else None
    if shape is None:
        shape = (int(rows.max()) + 1 if rows.size else 0, int(cols.max()) + 1 if cols.size else 0)
    return rows, cols, shape


def _row_labels(label_file, n_rows, what):
    labels = _read_labels(label_file)
    if len(labels) < n_rows:
        raise ValueError('%s holds %d labels, the table has %d %s rows' % (label_file, len(labels), n_rows, what))
    return np.asarray(labels[:n_rows], dtype=str)


def _thresholds(genomes_num):
    """uint32 thresholds of `count >= x` on the rows of the reference's count frame, which holds only rows with an entry:
    ceil(x), at least 1, at most what a count can be compared with (NaN: never met)."""
    out = []
    for x in genomes_num:
        x = float(x)
        if math.isnan(x) or x > 0xFFFFFFFF:
            out.append(0xFFFFFFFF)
        else:
            out.append(max(int(math.ceil(x)), 1))
    if not 1 <= len(out) <= _MAX_THRESHOLDS:
        raise ValueError('1 to %d thresholds are served by one call, not %d' % (_MAX_THRESHOLDS, len(out)))
    return np.asarray(out, dtype=np.uint32)


def _allele_groups(gene_labels, allele_labels):
    """(run_start, gene_of_run, new_row, old_row) for pgx_core_select: the allele rows grouped by gene name, whatever their
    order (pangenome._runs_by_name). The gene name is the reference's -- the first maximal run of characters other than
    `A` -- wherever that gives every allele row a gene; else the name is cut at the LAST `A` (__get_gene_from_allele__),
    as the builder and validate_gene_table do."""
    from .pangenome import _genes_of_alleles, _runs_by_name
    if allele_labels.size:
        first_a = pd.Series(allele_labels, dtype=object).str.extract(r'([^A]+)')[0]
        names = first_a.fillna('').values.astype(str)
        if not (first_a.notna().all() and np.isin(names, gene_labels).all()):
            names = _genes_of_alleles(allele_labels)
    else:
        names = allele_labels
    _, run_start, gene_of_run, new_row = _runs_by_name(gene_labels, names)
    old_row = np.empty(new_row.size, dtype=np.int64)
    old_row[new_row] = np.arange(new_row.size)
    return run_start, gene_of_run, new_row, old_row


def _select(who, ctx, a_rows, a_cols, a_shape, allele_labels, gene_labels, thresholds, g_rows=None, g_cols=None):
    """(names per threshold, gene_count of the gene rows): the one library call of both workflows."""
    n_alleles, n_genomes = a_shape
    if n_alleles and np.bincount(a_rows, minlength=n_alleles).min() == 0:
        raise ValueError(who + ': an allele row without any entry (the reference counts by position and would read '
                         'shifted rows)')
    run_start, gene_of_run, new_row, old_row = _allele_groups(gene_labels, allele_labels)
    if run_start.size == 1:
        return [np.zeros(0, dtype=allele_labels.dtype) for _ in thresholds], np.zeros(0, dtype=np.uint32)
    ctx = ctx or _native.default_context()
    out, dups = ctx.core_select(new_row[a_rows] if a_rows.size else a_rows, a_cols, n_alleles, n_genomes, run_start, thresholds,
                                gene_rows=g_rows, gene_genomes=g_cols, n_genes=gene_labels.size, gene_of_run=gene_of_run,
                                want=('gene_count', 'selected', 'n_selected'))
    if any(dups):
        raise ValueError(who + ' needs tables without duplicate entries')
    return [allele_labels[old_row[sel]] for sel in out['selected']], out['gene_count'][:gene_labels.size]


def _core_tables(allele_npz_file, allele_npz_label_file, gene_npz_file, gene_npz_label_file):
    a_rows, a_cols, a_shape = _load_coo(allele_npz_file)
    g_rows, g_cols, g_shape = _load_coo(gene_npz_file)
    if a_shape[1] != g_shape[1]:
        raise ValueError('the allele table has %d genomes, the gene table %d' % (a_shape[1], g_shape[1]))
    allele_labels = _row_labels(allele_npz_label_file, a_shape[0], 'allele')
    gene_labels = _row_labels(gene_npz_label_file, g_shape[0], 'gene')
    return a_rows, a_cols, a_shape, allele_labels, gene_labels, g_rows, g_cols


def core_allele_sets(allele_npz_file, allele_npz_label_file, gene_npz_file, gene_npz_label_file, genomes_nums, ctx=None):
    """For every threshold of genomes_nums (1 to 32 of them): the names of the most common allele of every gene held by
    at least that many genomes, in gene order -- what find_allele_names returns at the end of the reference's chain, as
    an array. One pass over the tables on the device (csrc/select.hip); writes and prints nothing. A threshold nobody
    meets gives an empty array."""
    thresholds = _thresholds(genomes_nums)
    tables = _core_tables(allele_npz_file, allele_npz_label_file, gene_npz_file, gene_npz_label_file)
    names, _ = _select('core_allele_sets', ctx, *tables[:5], thresholds=thresholds, g_rows=tables[5], g_cols=tables[6])
    return names


def create_core_genes_fasta(allele_npz_file, allele_npz_label_file, gene_npz_file, gene_npz_label_file, input_faa, genomes_num,
                            output_faa, ctx=None):
    """The most common allele of every gene held by at least genomes_num genomes, as a FASTA file (reference :7-26, with
    its printed lines). genomes_num and output_faa may be sequences of equal length (1 to 32): all thresholds are then
    served by one pass over the tables on the device and one pass over input_faa, and the last two lines are printed once
    per threshold. A float threshold means count >= x. When no gene meets a threshold: KeyError('gene_index') as in the
    reference, before anything is written (for any of the thresholds)."""
    many = np.ndim(genomes_num) > 0
    nums = list(genomes_num) if many else [genomes_num]
    outputs = list(output_faa) if many else [output_faa]
    if many and (isinstance(output_faa, str) or len(outputs) != len(nums)):
        raise ValueError('genomes_num and output_faa must be sequences of equal length')
    thresholds = _thresholds(nums)
    tables = _core_tables(allele_npz_file, allele_npz_label_file, gene_npz_file, gene_npz_label_file)
    names, gene_count = _select('create_core_genes_fasta', ctx, *tables[:5], thresholds=thresholds, g_rows=tables[5],
                                g_cols=tables[6])
    print("\nCounted allele occurence")
    print("\nIdentified all alleles per genome")
    print("\nCounted gene occurence")
    top = int(gene_count.max()) if gene_count.size else 0
    for t in range(thresholds.size):
        if top < int(thresholds[t]):
            raise KeyError('gene_index')                    # find_core_genes' frame has no columns
        if names[t].size == 0:
            raise KeyError('gene')                          # ... find_highest_allele_expression's has none
    for t in range(thresholds.size):
        print("\nFound the alleles with the highest expression per gene")
        print("\nCreated a FASTA file with all the highly expressed alleles. Success!")
    _filter_fasta(input_faa, names, outputs)
