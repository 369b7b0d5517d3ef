#!/usr/bin/env python
"""Golden fixtures for the direct UTR table validators, produced by RUNNING THE REFERENCE in the build container (needs
/root/reference; it never travels to the GPU box):

    python tests/golden/make_golden_proximal_direct.py

  pangenome.validate_proximal_table_direct   pangenome.py:1573-1647   (the two wrappers :1549-1570 call an undefined name
                                             and always raise NameError, so the direct function is what is recorded)

Inputs are the genomes, non-redundant FASTAs and tables of tests/golden/proximal (themselves reference output), used in
place, plus small variants written here under tests/golden/proximal_direct/<case>/. cases.json holds, per case: the genome
FNAs in the caller's order and the nr FASTA (paths relative to tests/golden), the table as labels and present cells (the
reference gets a pandas frame with NaN for absent cells), limits, side, log_group, and what the reference did: its stdout
(the golden directory written as <golden>) and, where it raised, the exception's type and argument.

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
from pangenomix_amd import sparse_utils                   # noqa: E402  (reads the .npz tables of tests/golden/proximal)

OUT = os.path.join(HERE, 'proximal_direct')
BASE = ['proximal/in/p1.fna', 'proximal/in/p2.fna', 'proximal/in/p10.fna']
COMP = str.maketrans('ACGTWSRYMKNacgtwsrymkn', 'TGCAWSYRKMNtgcawsyrkmn')


def rc(s):
    return s.translate(COMP)[::-1]


def read_fasta(path):
    out, name = {}, None
    for line in open(path):
        if line[0] == '>':
            name = line[1:].strip()
            out[name] = ''
        else:
            out[name] += line.strip()
    return out


class Case(object):
    """A table (labels + present cells), an nr FASTA and genome files, all editable before the reference runs."""

    def __init__(self, tag, limits, side, log_group=1, genomes=BASE):
        sub = {'up': ('upstream', 'Test', 'upstream'), 'down': ('downstream', 'Test', 'downstream'),
               'ov5': ('upstream_ov5', 'O', 'upstream')}[tag]
        exp = os.path.join(HERE, 'proximal', 'expected', sub[0])
        self.nr_base = 'proximal/expected/%s/%s_nr_%s.fna' % sub
        lsdf = sparse_utils.read_lsdf(os.path.join(exp, '%s_strain_by_%s.npz' % (sub[1], sub[2])))
        coo = lsdf.data.tocoo()
        self.index, self.columns = [str(x) for x in lsdf.index], [str(x) for x in lsdf.columns]
        self.cells = sorted(zip(coo.row.tolist(), coo.col.tolist()))
        self.nr = read_fasta(os.path.join(HERE, self.nr_base))
        self.nr_changed = False
        self.limits, self.side, self.log_group, self.genomes = list(limits), side, log_group, list(genomes)
        self.files = {}                                   # file name -> text, written under <case>/

    def add_row(self, label, seq, genomes, at=None):
        """A new row `label` with sequence `seq`, present in `genomes` (column labels); at = its position in the index."""
        at = len(self.index) if at is None else at
        self.cells = [(r + (r >= at), c) for r, c in self.cells]
        self.index.insert(at, label)
        self.cells = sorted(self.cells + [(at, self.columns.index(g)) for g in genomes])
        if seq is not None:
            self.nr[label] = seq
            self.nr_changed = True

    def genome_file(self, case, name, contigs):
        text = ''.join('>%s\n%s\n' % (c, '\n'.join(s[i:i + 70] for i in range(0, len(s), 70))) for c, s in contigs)
        self.files[name] = text
        return 'proximal_direct/%s/%s' % (case, name)


def contigs_of(g):
    return [(h.split()[0], s) for h, s in read_fasta(os.path.join(HERE, 'proximal', 'in', g + '.fna')).items()]


def build_cases():
    cases = {}
    for tag, limits, side in (('up', (-50, 3), 'upstream'), ('down', (-3, 50), 'downstream')):
        for lg in (1, 2):
            cases['%s_consistent_lg%d' % (tag, lg)] = Case(tag, limits, side, lg)
    p1 = dict(contigs_of('p1'))
    absent = 'ACGT' * 13 + 'A'                            # 53 nt that occur in no genome
    absent2 = 'TTGCA' * 10 + 'CCC'

    c = cases['up_cell_for_a_sequence_the_genome_lacks'] = Case('up', (-50, 3), 'upstream')
    r = c.index.index('T_C10U2')                          # p10's variant, claimed for p1 as well
    c.cells = sorted(set(c.cells) | {(r, c.columns.index('p1'))})

    c = cases['up_two_genes_share_a_sequence'] = Case('up', (-50, 3), 'upstream')
    c.add_row('T_C98U0', absent, ['p1', 'p2'], at=0)      # first place ...
    c.add_row('T_C97U0', absent2, ['p1'], at=3)
    c.add_row('T_C99U0', absent, ['p1'])                  # ... last name; p2 has only the first
    c.add_row('T_C96U0', c.nr['T_C11U0'], ['p1', 'p2', 'p10'])   # a shared sequence that IS there

    c = cases['even_window_palindrome_no_tally'] = Case('up', (-50, 2), 'upstream')
    half = 'GATTACAGGCTTAACGTCCATGAGCA'
    pal = half + rc(half)                                 # 52 nt, its own reverse complement
    half2 = 'CCATTGGACGTTAGCATCAGGATACT'
    c.index, c.cells, c.nr, c.nr_changed = [], [], {}, True
    g = c.genome_file('even_window_palindrome_no_tally', 'p1.fna', [('c1', p1['c1'][:300] + pal + p1['c1'][300:600])])
    c.genomes = [g]
    c.add_row('T_C1U0', pal, ['p1'])
    c.add_row('T_C2U0', half2 + rc(half2), ['p1'])        # a palindrome the genome lacks
    c.add_row('T_C3U0', p1['c1'][100:152], ['p1'])
    c.add_row('T_C4U0', rc(p1['c1'][400:452]), ['p1'])

    c = cases['odd_window_palindrome'] = Case('up', (-50, 3), 'upstream')
    pal53 = half + 'W' + rc(half)                         # W is its own complement
    c.index, c.cells, c.nr, c.nr_changed = [], [], {}, True
    c.genomes = [c.genome_file('odd_window_palindrome', 'p2.fna', [('c1', p1['c1'][:200] + pal53 + p1['c1'][200:400])])]
    c.add_row('T_C1U0', pal53, ['p2'])
    c.add_row('T_C2U0', half + 'S' + rc(half), ['p2'])

    cases['fragments_consistent'] = Case('ov5', (-50, 3), 'upstream')
    c = cases['fragments_suffix_rcprefix_neither'] = Case('ov5', (-50, 3), 'upstream')
    c.add_row('O_C90U0', p1['c1'][-30:], ['p1'])          # a contig's suffix: found
    c.add_row('O_C91U0', rc(p1['c2'][:25]), ['p1'])       # the reverse complement of a contig's prefix: found
    c.add_row('O_C92U0', p1['c1'][400:430], ['p1'])       # neither: missing, although it occurs
    c.add_row('O_C93U0', p1['c1'][:30], ['p1'])           # a prefix: missing
    c.add_row('O_C94U0', rc(p1['c2'][-30:]), ['p1'])      # reverse complement of a suffix: missing

    c = cases['sequence_longer_than_the_window'] = Case('up', (-50, 3), 'upstream')
    c.add_row('T_C90U0', p1['c1'][300:360], ['p1', 'p2'])
    c.add_row('T_C91U0', p1['c1'][-60:], ['p1'])

    c = cases['contig_shorter_than_the_window'] = Case('up', (-50, 3), 'upstream')
    short = 'GGATCCTTAGCATGCAAGTC'
    g = c.genome_file('contig_shorter_than_the_window', 'p1.fna', [('c0', short)] + contigs_of('p1') + [('c3', 'ACG')])
    c.genomes = [g] + BASE[1:]
    c.add_row('T_C90U0', short[-10:], ['p1'])             # suffix of the short contig
    c.add_row('T_C91U0', short, ['p1'])                   # the whole short contig
    c.add_row('T_C92U0', rc(short[:7]), ['p1'])
    c.add_row('T_C93U0', short[:10], ['p1'])              # missing
    c.add_row('T_C94U0', short + 'A' * 33, ['p1'])        # 53 nt that begin with the short contig: missing

    c = cases['lower_case_contigs'] = Case('up', (-50, 3), 'upstream')
    g = c.genome_file('lower_case_contigs', 'p1.fna', [(n, s.lower()) for n, s in contigs_of('p1')])
    c.genomes = [g] + BASE[1:]
    c.add_row('T_C90U0', p1['c1'][600:653].lower(), ['p1'])
    c.add_row('T_C91U0', rc(p1['c2'][100:153]).lower(), ['p1', 'p2'])

    c = cases['contig_with_unknown_bases'] = Case('up', (-50, 3), 'upstream', genomes=BASE)
    p2 = contigs_of('p2')
    s1, s2 = list(p2[0][1]), list(p2[1][1])
    s1[700], s1[880], s2[5] = 'X', 'Z', 'Q'               # away from every recorded sequence; X comes first
    g = c.genome_file('contig_with_unknown_bases', 'p2.fna', [('c1', ''.join(s1)), ('c2', ''.join(s2))])
    c.genomes = [BASE[0], g, BASE[2]]
    c.add_row('T_C90U0', absent, ['p1', 'p2'])            # missing from p1 (printed) and from p2 (never printed)

    c = cases['genome_absent_from_the_table'] = Case('down', (-3, 50), 'downstream')
    g = c.genome_file('genome_absent_from_the_table', 'p7.fna', contigs_of('p1'))
    c.genomes = [BASE[0], g, BASE[1]]

    c = cases['row_label_absent_from_the_nr_fasta'] = Case('down', (-3, 50), 'downstream')
    c.add_row('T_C90D0', None, ['p2'])                    # (the nr FASTA does not get the new label)

    cases['up_limits_50_5'] = Case('up', (-50, 5), 'upstream')
    cases['down_limits_5_50'] = Case('down', (-5, 50), 'downstream')
    cases['up_no_tally_limits_51_2'] = Case('up', (-51, 2), 'upstream')
    cases['down_no_tally_limits_2_51'] = Case('down', (-2, 51), 'downstream')
    cases['up_table_read_as_downstream'] = Case('up', (-50, 3), 'downstream')      # side and limits disagree: stop codons at [47:50]
    return cases


def main():
    if os.path.exists(OUT):
        shutil.rmtree(OUT)
    os.makedirs(OUT)
    record = {}
    for name, c in build_cases().items():
        nr_path = c.nr_base
        if c.nr_changed or c.files:
            os.makedirs(os.path.join(OUT, name), exist_ok=True)
        if c.nr_changed:
            nr_path = 'proximal_direct/%s/nr.fna' % name
            with open(os.path.join(HERE, nr_path), 'w') as f:
                for label, seq in c.nr.items():
                    f.write('>%s\n%s\n' % (label, seq))
        for fname, text in c.files.items():
            with open(os.path.join(OUT, name, fname), 'w') as f:
                f.write(text)
        values = np.full((len(c.index), len(c.columns)), np.nan)
        for r, col in c.cells:
            values[r, col] = 1.0
        df = pd.DataFrame(values, index=c.index, columns=c.columns)
        buf, exc = io.StringIO(), None
        try:
            with contextlib.redirect_stdout(buf):
                ref_pg.validate_proximal_table_direct(df, [os.path.join(HERE, g) for g in c.genomes],
                                                      os.path.join(HERE, nr_path), tuple(c.limits), c.side, c.log_group)
        except Exception as e:                            # recorded, not handled: the validators must raise the same
            exc = {'type': type(e).__name__, 'arg': e.args[0]}
        record[name] = {'genomes': c.genomes, 'nr': nr_path, 'index': c.index, 'columns': c.columns,
                        'cells': [list(x) for x in c.cells], 'limits': c.limits, 'side': c.side, 'log_group': c.log_group,
                        'stdout': buf.getvalue().replace(HERE, '<golden>'), 'exception': exc}
    with open(os.path.join(OUT, 'cases.json'), 'w') as f:
        json.dump(record, f, indent=0, sort_keys=True)
    print('proximal_direct: %d cases, %d with an exception, %d Missing lines' % (
        len(record), sum(r['exception'] is not None for r in record.values()),
        sum(r['stdout'].count('\tMissing') for r in record.values())))


if __name__ == '__main__':
    main()
