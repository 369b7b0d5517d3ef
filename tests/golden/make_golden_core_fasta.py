#!/usr/bin/env python
"""Golden fixtures for the two FASTA workflows of the reference's README ("EggNOG-mapper: prepare input fasta" and "Core
and accessory genome"), produced by RUNNING THE REFERENCE in the build container (needs /root/reference; it never travels
to the GPU box):

    python tests/golden/make_golden_core_fasta.py

  core_genome.create_core_genes_fasta            core_genome.py:7-26 and every helper it chains (:28-219)
  allele_identification.create_alleles_fasta     allele_identification.py:7-20 and its helpers (:24-157)

Both modules import Bio.SeqIO (Biopython), which is not installed. As in make_golden_next.py a placeholder module is
registered under that name; here it is NOT empty: parse() and write() below restate what Biopython's FASTA reader and
writer do to a record that is read and written back --
  reader  a record starts at a line beginning with '>'; its title is the rest of that line, right-stripped; id = the
          first whitespace-separated word of the title; the sequence is the following lines up to the next '>' with all
          blanks removed; whatever precedes the first '>' is skipped
  writer  '>' + title, then the sequence in lines of 60 (no line at all for an empty sequence)
-- so the files under tests/golden/core_fasta are the reference's code on top of these rules, NOT pinned against the real
library.

Cases (tests/golden/core_fasta/<case>/): the input tables, label files and FASTA file where they are not those of
tests/golden/cds/expected; `result.json` with the frames every helper returned (columns, dtypes, index, values), the
printed text and the exception, if any; the FASTA files written.
  cds_core_1, cds_core_3, cds_core_7   create_core_genes_fasta on the cds/expected tables; nobody meets 7: KeyError
  cds_alleles                          create_alleles_fasta on the same tables with an 'A' in front of every genome label
                                       (with the labels as they are the reference raises KeyError in .loc: recorded too)
  hand_core_<k>, hand_alleles          a hand-made table: ties (first allele wins), a gene whose allele rows are not
                                       contiguous, a gene with one allele, a gene row without alleles; FASTA ids with
                                       '|...' suffixes and descriptions, sequences of 0, 59, 60, 61, 121 residues, input
                                       wrapped at 70 columns, a record given twice, a record nobody asks for
  name_a_core_2, name_a_alleles        the table name contains 'A' (PAO1): the reference run with that letter replaced by
                                       'X' throughout, names mapped back
"""
import contextlib
import io
import json
import os
import shutil
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, '/root/reference')
sys.path.insert(0, '/root/reference/pangenomix')


class _Record(object):
    def __init__(self, title, seq):
        self.description = title
        self.id = title.split(None, 1)[0] if title.split() else ''
        self.seq = seq


def _parse(path, fmt):
    assert fmt == 'fasta'
    title, parts = None, []
    with open(path) as f:
        for line in f:
            if line[0] == '>':
                if title is not None:
                    yield _Record(title, ''.join(parts))
                title, parts = line[1:].rstrip(), []
            elif title is not None:
                parts.append(''.join(line.split()))
    if title is not None:
        yield _Record(title, ''.join(parts))


def _write(records, path, fmt):
    assert fmt == 'fasta'
    n = 0
    with open(path, 'w') as f:
        for rec in records:
            f.write('>' + rec.description + '\n')
            for i in range(0, len(rec.seq), 60):
                f.write(rec.seq[i:i + 60] + '\n')
            n += 1
    return n


for _name in ('Bio', 'Bio.SeqIO'):
    sys.modules.setdefault(_name, types.ModuleType(_name))
sys.modules['Bio'].SeqIO = sys.modules['Bio.SeqIO']
sys.modules['Bio.SeqIO'].parse = _parse
sys.modules['Bio.SeqIO'].write = _write

import pangenomix.core_genome as ref_cg                   # noqa: E402
import pangenomix.allele_identification as ref_ai         # noqa: E402

OUT = os.path.join(HERE, 'core_fasta')
CDS = os.path.join(HERE, 'cds', 'expected')


def frame(x):
    """A DataFrame or Series as JSON: what a test needs to compare it quirk for quirk."""
    import pandas as pd
    if isinstance(x, pd.Series):
        return {'kind': 'series', 'name': x.name, 'dtype': str(x.dtype), 'index': [int(i) for i in x.index],
                'index_dtype': str(x.index.dtype), 'values': x.tolist()}
    return {'kind': 'frame', 'columns': list(x.columns), 'dtypes': [str(t) for t in x.dtypes],
            'index': [int(i) for i in x.index], 'index_dtype': str(x.index.dtype),
            'index_class': type(x.index).__name__, 'values': json.loads(x.to_json(orient='values'))}


def run_steps(steps, result):
    """steps: [(name, callable(env) -> value)]; records each frame, all printed text, and the exception that ends it"""
    env, buf = {}, io.StringIO()
    result['frames'] = {}
    result['raises'] = None
    with contextlib.redirect_stdout(buf):
        for name, fn in steps:
            try:
                env[name] = fn(env)
            except Exception as e:                          # noqa: BLE001 (recorded, whatever it is)
                result['raises'] = {'type': type(e).__name__, 'args': [str(a) for a in e.args], 'step': name}
                break
            if env[name] is not None:
                result['frames'][name] = frame(env[name])
    result['stdout_steps'] = buf.getvalue()
    return env


def core_case(case, files, genomes_num, rename=None):
    """files: allele npz, allele labels, gene npz, gene labels, input faa"""
    a_npz, a_lab, g_npz, g_lab, faa = files
    d = os.path.join(OUT, case)
    os.makedirs(d, exist_ok=True)
    result = {'genomes_num': genomes_num}
    steps = [
        ('count_allele_occurence', lambda e: ref_cg.count_allele_occurence(a_npz)),
        ('identify_gene_allele_rows', lambda e: ref_cg.identify_gene_allele_rows(g_lab, a_lab)),
        ('count_gene_occurence', lambda e: ref_cg.count_gene_occurence(g_npz)),
        ('find_core_genes', lambda e: ref_cg.find_core_genes(e['count_gene_occurence'], genomes_num)),
        ('subset_genes_alleles_pairs',
         lambda e: ref_cg.subset_genes_alleles_pairs(e['identify_gene_allele_rows'], e['find_core_genes'])),
        ('find_highest_allele_expression',
         lambda e: ref_cg.find_highest_allele_expression(e['count_allele_occurence'], e['subset_genes_alleles_pairs'])),
        ('find_allele_names', lambda e: ref_cg.find_allele_names(e['find_highest_allele_expression'].copy(), a_lab)),
    ]
    run_steps(steps, result)
    out_faa = os.path.join(d, 'out.faa')
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        try:
            ref_cg.create_core_genes_fasta(a_npz, a_lab, g_npz, g_lab, faa, genomes_num, out_faa)
            result['raises_whole'] = None
        except Exception as e:                              # noqa: BLE001
            result['raises_whole'] = {'type': type(e).__name__, 'args': [str(a) for a in e.args]}
    result['stdout'] = buf.getvalue()
    result['wrote'] = os.path.exists(out_faa)
    finish(d, result, rename)


def alleles_case(case, files, rename=None, also_raw=None):
    a_npz, a_lab, g_lab, faa = files
    d = os.path.join(OUT, case)
    os.makedirs(d, exist_ok=True)
    result = {}
    steps = [
        ('count_allele_occurence', lambda e: ref_ai.count_allele_occurence(a_npz)),
        ('identify_gene_allele_rows', lambda e: ref_ai.identify_gene_allele_rows(g_lab, a_lab)),
        ('find_highest_expression',
         lambda e: ref_ai.find_highest_expression(e['count_allele_occurence'], e['identify_gene_allele_rows'])),
        ('find_allele_names', lambda e: ref_ai.find_allele_names(e['find_highest_expression'].copy(), a_lab)),
    ]
    run_steps(steps, result)
    out_faa = os.path.join(d, 'out.faa')
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        ref_ai.create_alleles_fasta(a_npz, g_lab, a_lab, faa, out_faa)
    result['stdout'] = buf.getvalue()
    result['wrote'] = True
    if also_raw:                                            # the reference on the labels as they are
        ra_lab, rg_lab = also_raw
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                ref_ai.create_alleles_fasta(a_npz, rg_lab, ra_lab, faa, os.path.join(d, 'raw.faa'))
            result['raw_raises'] = None
        except Exception as e:                              # noqa: BLE001
            result['raw_raises'] = {'type': type(e).__name__, 'args': [str(a) for a in e.args]}
        if os.path.exists(os.path.join(d, 'raw.faa')):
            os.remove(os.path.join(d, 'raw.faa'))
    finish(d, result, rename)


def finish(d, result, rename):
    text = json.dumps(result, sort_keys=True)
    if rename:
        text = text.replace(rename[0], rename[1])
        out_faa = os.path.join(d, 'out.faa')
        if os.path.exists(out_faa):
            with open(out_faa) as f:
                body = f.read()
            with open(out_faa, 'w') as f:
                f.write(body.replace(rename[0], rename[1]))
    with open(os.path.join(d, 'result.json'), 'w') as f:
        f.write(text + '\n')


def relabel_genomes(src, dst, n_genomes):
    with open(src) as f:
        lines = f.read().split('\n')
    assert lines[-1] == ''
    body = lines[:-1]
    body = body[:len(body) - n_genomes] + ['A' + x for x in body[len(body) - n_genomes:]]
    with open(dst, 'w') as f:
        f.write('\n'.join(body) + '\n')


def save_table(path, rows_of, n_rows, n_genomes, labels, genomes):
    """An LSDF .npz in the reference's format plus its label file (row labels, then genome labels)."""
    row = np.array([r for r, cols in enumerate(rows_of) for _ in cols], dtype=np.int32)
    col = np.array([c for cols in rows_of for c in cols], dtype=np.int32)
    order = np.lexsort((row, col))                           # column-major, as the builder leaves it
    np.savez_compressed(path, row=row[order], col=col[order], format=np.bytes_('coo'),
                        shape=np.array([n_rows, n_genomes], dtype=np.int64), data=np.ones(row.size, dtype=np.int64))
    with open(path + '.labels.txt', 'w') as f:
        f.write('\n'.join(list(labels) + list(genomes)) + '\n')


def wrap70(seq):
    return ''.join(seq[i:i + 70] + '\n' for i in range(0, len(seq), 70))


def make_hand(d, name):
    """The hand-made tables and FASTA file under directory d, for table name `name`; returns the paths."""
    os.makedirs(d, exist_ok=True)
    genomes = ['s1', 's2', 's3', 's4', 's5']
    alleles = ['C0A0', 'C0A1', 'C1A0', 'C0A2', 'C2A0', 'C1A1', 'C4A0', 'C4A1']
    a_cols = [[0, 1], [2, 3], [0], [4], [0, 1, 2, 3], [1, 2, 3], [0, 1], [2, 3]]
    genes = ['C0', 'C1', 'C2', 'C3', 'C4']
    g_cols = [[0, 1, 2, 3, 4], [0, 1, 2, 3], [0, 1, 2, 3], [0, 1], [0, 1, 2, 3]]
    a_npz, g_npz = os.path.join(d, name + '_strain_by_allele.npz'), os.path.join(d, name + '_strain_by_gene.npz')
    save_table(a_npz, a_cols, len(alleles), len(genomes), [name + '_' + a for a in alleles], genomes)
    save_table(g_npz, g_cols, len(genes), len(genomes), [name + '_' + g for g in genes], genomes)
    rng = np.random.default_rng(5)
    aa = np.array(list('ACDEFGHIKLMNPQRSTVWY'))
    lengths = dict(zip(alleles, [0, 59, 60, 61, 121, 10, 70, 5]))
    seqs = {a: ''.join(rng.choice(aa, n)) for a, n in lengths.items()}
    faa = os.path.join(d, name + '_nr.faa')
    with open(faa, 'w') as f:
        def rec(title, seq):
            f.write('>' + title + '\n' + wrap70(seq))
        rec('%s_C0A0|fig|1.1.peg.1 hypothetical protein  ' % name, seqs['C0A0'])
        rec('%s_C0A1' % name, seqs['C0A1'])
        rec('%s_C1A0|x' % name, seqs['C1A0'])
        rec('%s_C9A0|nobody asks for this one' % name, 'MKV')
        rec('%s_C0A2 a description | with a bar' % name, seqs['C0A2'])
        rec('%s_C2A0|fig|1.1.peg.7\tDNA polymerase' % name, seqs['C2A0'])
        rec('%s_C1A1|y z' % name, seqs['C1A1'])
        rec('%s_C4A0' % name, seqs['C4A0'])
        rec('%s_C4A1' % name, seqs['C4A1'])
        rec('%s_C2A0|fig|2.2.peg.9 given twice' % name, seqs['C2A0'][:61])
        rec('%s_C1A1x|a longer id' % name, 'MK')
    return a_npz, a_npz + '.labels.txt', g_npz, g_npz + '.labels.txt', faa


def main():
    if os.path.exists(OUT):
        shutil.rmtree(OUT)
    os.makedirs(OUT)
    cds = (os.path.join(CDS, 'T_strain_by_allele.npz'), os.path.join(CDS, 'T_strain_by_allele.npz.labels.txt'),
           os.path.join(CDS, 'T_strain_by_gene.npz'), os.path.join(CDS, 'T_strain_by_gene.npz.labels.txt'),
           os.path.join(CDS, 'T_nr.faa'))
    for k in (1, 3, 7):
        core_case('cds_core_%d' % k, cds, k)
    d = os.path.join(OUT, 'cds_alleles')
    os.makedirs(d)
    relabel_genomes(cds[1], os.path.join(d, 'allele_labels_A.txt'), 6)
    relabel_genomes(cds[3], os.path.join(d, 'gene_labels_A.txt'), 6)
    alleles_case('cds_alleles', (cds[0], os.path.join(d, 'allele_labels_A.txt'), os.path.join(d, 'gene_labels_A.txt'), cds[4]),
                 also_raw=(cds[1], cds[3]))

    hand = make_hand(os.path.join(OUT, 'hand_in'), 'H')
    for k in (1, 3, 5, 6):
        core_case('hand_core_%d' % k, hand, k)
    d = os.path.join(OUT, 'hand_alleles')
    os.makedirs(d)
    relabel_genomes(hand[1], os.path.join(d, 'allele_labels_A.txt'), 5)
    relabel_genomes(hand[3], os.path.join(d, 'gene_labels_A.txt'), 5)
    alleles_case('hand_alleles', (hand[0], os.path.join(d, 'allele_labels_A.txt'), os.path.join(d, 'gene_labels_A.txt'), hand[4]),
                 also_raw=(hand[1], hand[3]))

    make_hand(os.path.join(OUT, 'name_a_in'), 'PAO1')        # what the tests read
    tmp = os.path.join(OUT, '_tmp_PXO1')
    x = make_hand(tmp, 'PXO1')                               # what the reference can group
    core_case('name_a_core_2', x, 2, rename=('PXO1', 'PAO1'))
    d = os.path.join(OUT, 'name_a_alleles')
    os.makedirs(d)
    relabel_genomes(x[1], os.path.join(tmp, 'allele_labels_A.txt'), 5)
    relabel_genomes(x[3], os.path.join(tmp, 'gene_labels_A.txt'), 5)
    alleles_case('name_a_alleles', (x[0], os.path.join(tmp, 'allele_labels_A.txt'), os.path.join(tmp, 'gene_labels_A.txt'), x[4]),
                 rename=('PXO1', 'PAO1'))
    shutil.rmtree(tmp)
    n = sum(len(files) for _, _, files in os.walk(OUT))
    print('core_fasta: %d files under %s' % (n, os.path.relpath(OUT, HERE)))


if __name__ == '__main__':
    main()
