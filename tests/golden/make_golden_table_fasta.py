#!/usr/bin/env python
"""Golden fixtures for the table-against-FASTA validators, produced by RUNNING THE REFERENCE in the build container (needs
/root/reference; it never travels to the GPU box):

    python tests/golden/make_golden_table_fasta.py

  pangenome.validate_table_against_fasta   pangenome.py:1418-1546, through its three wrappers
  pangenome.validate_allele_table / validate_upstream_table / validate_downstream_table   :1333-1415

Inputs are the genomes, non-redundant FASTAs, names file and tables of tests/golden/cds and tests/golden/proximal
(themselves reference output), used in place, plus small files written here under tests/golden/table_fasta/ (quirks/ is
shared by the four quirks cases). cases.json holds the three tables used in place once ("tables": labels and the cells that
are 1) and, one line per case: which wrapper ran (kind), the genome files in the caller's order, the nr FASTA and the allele
names file (paths relative to tests/golden), the table -- either whole (index, columns, cells) or as a named table with the
labels appended to its index and the cells added to and removed from it -- the cells with any other value than 0 or 1
(None = NaN), log_group, and what the reference did: its stdout (the golden directory written as <golden>) and, where it
raised, the exception's type and argument. tests/dict_match_model.load_cases() expands every case to a whole table.

The imports the reference needs but never uses here are registered as empty placeholder modules (see make_golden_next.py).
"""
import contextlib
import io
import json
import os
import shutil
import sys
import types

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, '/root/reference')
sys.path.insert(0, '/root/reference/pangenomix')
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
for _name in ('statsmodels', 'statsmodels.stats', 'Bio', 'Bio.SeqIO'):
    sys.modules.setdefault(_name, types.ModuleType(_name))
sys.modules['statsmodels'].stats = sys.modules['statsmodels.stats']
sys.modules['Bio'].SeqIO = sys.modules['Bio.SeqIO']

import pangenomix.pangenome as ref_pg                     # noqa: E402
from pangenomix_amd import sparse_utils                   # noqa: E402  (reads the .npz tables of the other fixtures)

OUT = os.path.join(HERE, 'table_fasta')
CDS_GENOMES = ['cds/in/%s.faa' % g for g in ('g10', 'g2', 'gA', 'gB', 'gC.v1', 'gD')]


class Case(object):
    """A table (labels, cells), an nr FASTA, genome files and a names file, all editable before the reference runs."""

    def __init__(self, base=None, log_group=1):
        self.kind, self.names, self.log_group = 'allele', None, log_group
        self.index, self.columns, self.cells, self.other = [], [], [], []
        self.genomes, self.nr = [], None
        self.files = {}                                   # path under table_fasta/ -> text
        self.base, self.base_index, self.base_cells = base, [], []
        if base == 'cds':
            self.table('cds/expected/T_strain_by_allele.npz')
            self.genomes, self.nr = list(CDS_GENOMES), 'cds/expected/T_nr.faa'
        elif base in ('upstream', 'downstream'):
            exp = 'proximal/expected/%s/' % base
            self.table(exp + 'Test_strain_by_%s.npz' % base)
            self.genomes = [exp + '%s_%s.fna' % (g, base) for g in ('p1', 'p2', 'p10')]
            self.nr, self.names, self.kind = exp + 'Test_nr_%s.fna' % base, 'proximal/in/T_allele_names.tsv', base

    def table(self, npz):
        lsdf = sparse_utils.read_lsdf(os.path.join(HERE, npz))
        coo = lsdf.data.tocoo()
        self.index, self.columns = [str(x) for x in lsdf.index], [str(x) for x in lsdf.columns]
        self.cells = sorted(zip(coo.row.tolist(), coo.col.tolist()))
        self.base_index, self.base_cells = list(self.index), list(self.cells)

    def cell(self, label, genome):
        return (self.index.index(label), self.columns.index(genome))

    def present(self, genome):
        return [self.index[r] for r, c in self.cells if c == self.columns.index(genome)]

    def absent(self, genome):
        have = set(self.present(genome))
        return [x for x in self.index if x not in have]

    def swap(self, genome, drop=1, add=1):
        """drop cells the genome has (they become genome-only records) and add cells it lacks (table-only)"""
        lacks = self.absent(genome)[:add]
        for label in self.present(genome)[:drop]:
            self.cells.remove(self.cell(label, genome))
        for label in lacks:
            self.cells.append(self.cell(label, genome))
        self.cells.sort()

    def file(self, directory, name, text):
        self.files['%s/%s' % (directory, name)] = text
        return 'table_fasta/%s/%s' % (directory, name)


QUIRKS_NR = ('LEADSEQ\n'                                  # lines before the first header: the record ''
             '>X_C0A0 some description\nACDEFG\nHIK\n'
             '>X_C1A0\nMMMM\n'
             '>X_C2A0\nMM\nMM\n'                          # the sequence of X_C1A0 again: COLLISION, the later header wins
             '>X_C3A0\n\n'                                # a blank line: the sequence ''
             '>X_C4A0\n'                                  # a header and no line: no record
             '>X_C5A0\t tabbed description \nWWWW\n'
             '>X_C6A0\n  PPPP  \n\tQQ')                   # stripped lines; no final newline
QUIRKS_Q1 = ('>a first\nACDEF\nGHIK\n'                    # X_C0A0's sequence, wrapped differently
             '>b\nMMMM\n'                                 # found under the later header X_C2A0
             '>c\nZZZZ\n'                                 # absent from the nr set
             '>d\n\n'                                     # the sequence '': X_C3A0
             '>e\n')                                      # no line: no record
QUIRKS_Q2 = ('LEAD\nSEQ\n'                                # a headerless leading sequence: the nr record ''
             '>x\nPPPPQQ\n>y\n>z\nWW\n WW')               # y has no line; no final newline


def quirks(name, cases):
    c = cases[name] = Case()
    c.nr = c.file('quirks', 'nr.faa', QUIRKS_NR)
    c.genomes = [c.file('quirks', 'q1.faa', QUIRKS_Q1), c.file('quirks', 'q2_footer.faa', QUIRKS_Q2)]
    c.index = ['X_C0A0', 'X_C1A0', 'X_C3A0', '', 'X_C5A0\t tabbed description', 'X_C6A0', 'X_C9A0']
    c.columns = ['q1', 'q2']
    # q1: X_C0A0 lacks the description (table only; the record's name is genome only), X_C1A0 is the earlier header of
    # the collision (table only, X_C2A0 -- no label at all -- genome only), X_C3A0 agrees
    # q2: everything agrees
    c.cells = sorted([c.cell('X_C0A0', 'q1'), c.cell('X_C1A0', 'q1'), c.cell('X_C3A0', 'q1'), c.cell('', 'q2'),
                      c.cell('X_C5A0\t tabbed description', 'q2'), c.cell('X_C6A0', 'q2')])
    return c


NAMES = ('Y_C1A0\tfig|u1.peg.1|tagA\tfig|u2.peg.1\n'      # a PATRIC feature with its locus tag
         'Y_C2A0\tfig|u1.peg.2\tfig|u2.peg.2\n'
         'T_C1A0\tfig|u1.peg.3\n'
         '_C1A0\tfig|u2.peg.3\n'
         'Y_C7A0\tfig|u2.peg.2\n'                         # fig|u2.peg.2 again: the last line wins
         'Y_C2A1\tfig|u2.peg.2\n')
UTR = 'TTGACATATAATGCTAGCAGGAGGTTTAAACATGAAACGTCTGATTGCACTGA'


def proximal(name, cases, side, letter):
    """conserved UTRs shared by two genes, which only the suffix tells apart; the pair 'ACG' + 'T_C1' = 'ACGT' + '_C1'"""
    c = cases[name] = Case()
    c.kind = side
    tag = '_%s(-50,3)' % side
    c.names = c.file(name, 'names.tsv', NAMES)
    c.nr = c.file(name, 'nr.fna', ''.join('>%s\n%s\n' % x for x in (
        ('Y_C1%s0' % letter, UTR), ('Y_C2%s0' % letter, UTR), ('T_C1%s0' % letter, 'ACG'), ('_C1%s0' % letter, 'ACGT'),
        ('Y_C8%s0' % letter, UTR[::-1]))))
    u1 = [('fig|u1.peg.1' + tag, UTR), ('fig|u1.peg.2' + tag, UTR), ('fig|u1.peg.3' + tag, 'ACG'),
          ('fig|u1.peg.9' + tag, UTR)]                    # peg.9 is in no names line: the bare sequence is no key
    u2 = [('fig|u2.peg.1' + tag, UTR), ('fig|u2.peg.2' + tag + ' trailing words', UTR[:30] + '\n' + UTR[30:]),
          ('fig|u2.peg.3' + tag, 'ACGT'), ('fig|u2.peg.4', UTR[::-1])]
    c.genomes = [c.file(name, 'u1_%s.fna' % side, ''.join('>%s\n%s\n' % x for x in u1)),
                 c.file(name, 'u2_%s.fna' % side, ''.join('>%s\n%s\n' % x for x in u2))]
    c.index = ['Y_C1%s0' % letter, 'Y_C2%s0' % letter, 'T_C1%s0' % letter, '_C1%s0' % letter, 'Y_C8%s0' % letter]
    c.columns = ['u1', 'u2']
    # u1 holds both genes' UTRs (equal sequences) and, for 'ACG' + 'T_C1', the later header _C1?0 where the table has T_C1?0
    c.cells = sorted([(0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (3, 1)])
    return c


def build_cases():
    cases = {}
    cases['cds_consistent'] = Case('cds')
    c = cases['cds_unsorted_paths_log_group_2'] = Case('cds', log_group=2)
    c.genomes = [c.genomes[i] for i in (3, 0, 5, 1, 4, 2)]
    c = cases['cds_one_genome_differs'] = Case('cds')
    c.swap('gB', drop=1, add=2)
    c = cases['cds_several_genomes_differ'] = Case('cds', log_group=2)
    c.swap('g10', drop=2, add=0)
    c.swap('gC.v1', drop=0, add=3)
    c.swap('gD', drop=1, add=1)
    c = cases['cds_frame_with_a_nan_and_a_2'] = Case('cds')
    r, col = c.cell(c.present('g2')[3], 'g2')
    c.cells.remove((r, col))
    c.other.append([r, col, 2])                           # not == 1: absent, the genome's record is genome only
    r, col = c.cell(c.absent('gA')[0], 'gA')
    c.other.append([r, col, None])                        # NaN: absent, as the genome has it
    c = cases['cds_duplicate_index_labels'] = Case('cds')
    have, lack = c.present('gA')[0], c.absent('gA')[0]
    c.index += [have, lack, lack]                         # rows with labels the table already has
    n = len(c.index)
    c.cells += [(n - 3, c.columns.index('gA')),           # a second row of a label gA has: counted once
                (n - 2, c.columns.index('gA')), (n - 1, c.columns.index('gA')),   # two rows of one gA lacks: table only 1
                (n - 3, c.columns.index('gB'))]
    c.cells.sort()
    cases['cds_no_genomes'] = Case('cds')
    cases['cds_no_genomes'].genomes = []
    quirks('quirks', cases)
    c = quirks('quirks_genome_without_a_column', cases)
    c.genomes.insert(1, c.file('quirks', 'q1b_x.faa', '>a\nMMMM\n'))
    c = quirks('quirks_missing_file', cases)
    c.genomes.insert(1, 'table_fasta/quirks/q1_absent.faa')
    c = quirks('quirks_missing_file_log_group_2', cases)
    c.log_group = 2
    c.genomes.append('table_fasta/quirks/q9.faa')
    for side, letter in (('upstream', 'U'), ('downstream', 'D')):
        cases[side + '_consistent'] = Case(side)
        c = cases[side + '_one_cell_flipped'] = Case(side, log_group=3)
        c.swap('p10', drop=1, add=1)
        proximal(side + '_shared_utrs_and_suffix_boundary', cases, side, letter)
    return cases


def main():
    if os.path.exists(OUT):
        shutil.rmtree(OUT)
    os.makedirs(OUT)
    record, tables = {}, {}
    for name, c in sorted(build_cases().items()):
        for fname, text in c.files.items():
            os.makedirs(os.path.dirname(os.path.join(OUT, fname)), exist_ok=True)
            with open(os.path.join(OUT, fname), 'w') as f:
                f.write(text)
        values = np.zeros((len(c.index), len(c.columns)))
        for r, col in c.cells:
            values[r, col] = 1.0
        for r, col, v in c.other:
            values[r, col] = np.nan if v is None else v
        df = pd.DataFrame(values, index=c.index, columns=c.columns)
        genomes = [os.path.join(HERE, g) for g in c.genomes]
        nr = os.path.join(HERE, c.nr)
        buf, exc = io.StringIO(), None
        try:
            with contextlib.redirect_stdout(buf):
                if c.kind == 'allele':
                    ref_pg.validate_allele_table(df, genomes, nr, c.log_group)
                else:
                    fn = ref_pg.validate_upstream_table if c.kind == 'upstream' else ref_pg.validate_downstream_table
                    fn(df, genomes, nr, os.path.join(HERE, c.names), c.log_group)
        except Exception as e:                            # recorded, not handled: the validators must raise the same
            exc = {'type': type(e).__name__, 'arg': e.args[0]}
        record[name] = {'kind': c.kind, 'genomes': c.genomes, 'nr': c.nr, 'allele_names': c.names, 'other': c.other,
                        'log_group': c.log_group, 'stdout': buf.getvalue().replace(HERE, '<golden>'), 'exception': exc}
        if c.base:
            assert c.index[:len(c.base_index)] == c.base_index
            tables[c.base] = {'index': c.base_index, 'columns': c.columns, 'cells': [list(x) for x in c.base_cells]}
            record[name].update(table=c.base, index_appended=c.index[len(c.base_index):],
                                cells_added=[list(x) for x in sorted(set(c.cells) - set(c.base_cells))],
                                cells_removed=[list(x) for x in sorted(set(c.base_cells) - set(c.cells))])
        else:
            record[name].update(table=None, index=c.index, columns=c.columns, cells=[list(x) for x in c.cells])
    dumps = lambda x: json.dumps(x, sort_keys=True, separators=(',', ':'))                        # noqa: E731
    with open(os.path.join(OUT, 'cases.json'), 'w') as f:                     # one line per table and per case
        f.write('{"tables":{\n' + ',\n'.join('%s:%s' % (dumps(k), dumps(v)) for k, v in sorted(tables.items())))
        f.write('\n},"cases":{\n' + ',\n'.join('%s:%s' % (dumps(k), dumps(v)) for k, v in sorted(record.items())) + '\n}}\n')
    print('table_fasta: %d cases, %d with an exception, %d inconsistent genomes, %d COLLISION lines' % (
        len(record), sum(r['exception'] is not None for r in record.values()),
        sum(r['stdout'].count('Table only:') for r in record.values()),
        sum(r['stdout'].count('COLLISION:') for r in record.values())))


if __name__ == '__main__':
    main()
