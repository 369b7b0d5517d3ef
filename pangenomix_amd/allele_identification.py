"""The reference's allele_identification module on MI355X, complete: allele occurrence counts, the most
common allele of every gene and the FASTA file of those alleles (create_alleles_fasta, the README's "EggNOG-mapper:
prepare input fasta" workflow). Same arguments, same DataFrames, same printed lines as reference
allele_identification.py:7-157; see core_genome.py, whose helpers these are, and INTEGRATION.md for the inputs on which
the reference itself fails (it does on any table whose genome labels hold no `A`)."""
from __future__ import print_function

import numpy as np

from . import core_genome
from .core_genome import _row_occurrence
from .core_genome import filter_sequences, find_allele_names, identify_gene_allele_rows          # noqa: F401 (the reference's names)


def count_allele_occurence(allele_npz_file, ctx=None):
    """Occurrence of each allele over all genomes (reference allele_identification.py:129-157)."""
    df = _row_occurrence(allele_npz_file, 'allele_index', ctx)
    print("\nCounted allele occurence")
    return df


def find_highest_expression(row_counts_df, gene_allele_rows_df):
    """The most common allele of every gene (reference :62-92): columns gene / highest_expression (int64), the first
    allele winning a tie; an empty frame without columns for no genes."""
    return core_genome._highest_expression(row_counts_df, gene_allele_rows_df)


def create_alleles_fasta(allele_npz_file, gene_npz_label_file, allele_npz_label_file, input_faa, output_faa, ctx=None):
    """The most common allele of every gene, as a FASTA file (reference :7-20, with its printed lines). One library call
    (csrc/select.hip) and one pass over input_faa. Genome labels are never rows here: the allele rows are the first
    shape[0] labels of the allele file, the gene rows the gene file's labels less the shape[1] genome labels at its end."""
    a_rows, a_cols, a_shape = core_genome._load_coo(allele_npz_file)
    allele_labels = core_genome._row_labels(allele_npz_label_file, a_shape[0], 'allele')
    gene_lines = core_genome._read_labels(gene_npz_label_file)
    if len(gene_lines) < a_shape[1]:
        raise ValueError('%s holds %d labels, the table has %d genomes' % (gene_npz_label_file, len(gene_lines), a_shape[1]))
    gene_labels = np.asarray(gene_lines[:len(gene_lines) - a_shape[1]], dtype=str)
    # every gene row counts (threshold 0, no gene table): a run is selected iff it has a gene row and an allele
    names, _ = core_genome._select('create_alleles_fasta', ctx, a_rows, a_cols, a_shape, allele_labels, gene_labels,
                                   thresholds=np.zeros(1, dtype=np.uint32))
    print("\nCounted allele occurence")
    print("\nIdentified all alleles per genome")
    if names[0].size == 0:
        raise KeyError('gene')                              # find_highest_expression's frame has no columns
    print("\nFound the alleles with the highest expression per gene")
    print("\nCreated a FASTA file with all the highly expressed alleles. Success!")
    core_genome._filter_fasta(input_faa, names, [output_faa])
