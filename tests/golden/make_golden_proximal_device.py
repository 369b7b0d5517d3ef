"""Writes tests/golden/proximal_device: what the reference's 5'/3' UTR builders (pangenome.py:743-1184) wrote, printed and raised
on small genomes that hold every case the device path of pangenomix_amd.pangenome (ctx=) has to reproduce or
to hand to the host. Needs the reference checkout (imported as tests/golden/make_golden_next.py does); nothing of it is
copied. Layout: in/ (GFF, FNA, allele names, hand-made extracts), expected/<run>/ (every file the run wrote: the
per-genome extracts, <name>_nr_<side>.fna, the .npz and its labels), expected/runs.json (per run: arguments, stdout, the
exception, the genomes the device path must leave to the host).

Genomes (limits (-20, 3) upstream, (-3, 20) downstream; windows of 23 bases):
  q1 q2 q3 q4 q10   the main set: contigs c1 (260), c2 (150), c3 (18: shorter than a window -- the negative-start slice).
                    q10's extract sorts before q1's ('q10_up' < 'q1_up': '0' < '_') while 'q1' < 'q10'.
  qx                q1 with a base outside the complement table in a minus-strand window: KeyError, partial extract
  qnc               q1 with a mapped tRNA line: fine without max_overlap, KeyError with it (its (start, stop) is no CDS)
  qcr qsp           q1 with \\r\\n line ends in the FNA / q2 with a blank inside a sequence line: host path by rule"""
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
for _name in ('statsmodels', 'statsmodels.stats', 'Bio', 'Bio.SeqIO'):
    sys.modules.setdefault(_name, types.ModuleType(_name))
sys.modules['statsmodels'].stats = sys.modules['statsmodels.stats']
sys.modules['Bio'].SeqIO = sys.modules['Bio.SeqIO']

import pangenomix.pangenome as ref_pg                     # noqa: E402

UP, DOWN = (-20, 3), (-3, 20)
# (contig, type, start, stop, strand, peg number, gene number); 1-based inclusive coordinates. Gene numbers 1, 10, 100, 2
# pin the string order of the rows; gene 100 has three paralogs per genome (12 variants over q1..q4: U10 against U2).
FEATS = [('c1', 'CDS', 8, 40, '+', 1, 1),        # upstream window cut off by the contig start
         ('c1', 'CDS', 46, 80, '+', 2, 10),      # 5 bases behind peg.1: truncated with max_overlap 0, whole with 5 ... 25
         ('c1', 'CDS', 84, 110, '+', 3, 2),      # 3 bases behind peg.2
         ('c1', 'tRNA', 112, 118, '+', None, None),
         ('c1', 'CDS', 120, 150, '-', 4, 3),     # minus strand: lower case, ambiguity codes and an N around it
         ('c1', 'CDS', 156, 190, '-', 5, 4),     # 5 bases behind peg.4 on the minus strand
         ('c1', 'CDS', 215, 252, '-', 6, 5),     # upstream (minus strand: to the right) cut off by the contig end
         ('c2', 'CDS', 30, 50, '+', 7, 100),
         ('c2', 'CDS', 78, 98, '+', 8, 100),     # a paralog of peg.7
         ('c2', 'CDS', 124, 128, '-', 9, 100),   # and another, on the other strand
         ('c2', 'CDS', 100, 120, '+', 10, 6),    # the window of peg.8's gene 100 copied here: one window, two genes
         ('c3', 'CDS', 6, 16, '+', 11, 7),       # contig shorter than the window: seq[-15:8]
         ('c9', 'CDS', 10, 100, '+', 12, 8),     # contig missing from the FNA
         ('c1', 'CDS', 194, 210, '+', 13, None)]  # not in the name table
MAIN = ['q1', 'q2', 'q3', 'q4', 'q10']


def base_contigs():
    rng = np.random.default_rng(2026)
    nt = np.array(list('ACGT'))
    c = {name: list(rng.choice(nt, n)) for name, n in (('c1', 260), ('c2', 150), ('c3', 18))}
    for at, b in ((152, 'a'), (153, 'c'), (154, 'n'), (155, 'N'), (157, 'R'), (158, 'y'), (160, 'W'), (161, 'k'), (162, 'M'),
                  (111, 's'), (113, 'g'), (114, 't'), (116, 'K'), (117, 'Y')):
        c['c1'][at] = b                           # around the minus-strand pegs 4 and 5
    same_window(c['c2'])
    return c


def same_window(c2):
    """the upstream window of peg.10 (gene 6, at 100) = the upstream window of peg.8 (gene 100, at 78); the two overlap in
    one base, so the copy is made twice"""
    for _ in range(2):
        c2[79:102] = c2[57:80]


def mutate(seq, at):
    seq[at] = 'A' if seq[at] != 'A' else 'C'


def write_genome(din, g, contigs, feats, line_end='\n', blank_at=None):
    with open(os.path.join(din, g + '.fna'), 'w', newline='') as f:
        for name, s in contigs.items():
            s = ''.join(s)
            lines = [s[i:i + 60] for i in range(0, len(s), 60)]
            if blank_at is not None and name == 'c1':
                lines[blank_at] = lines[blank_at][:30] + ' ' + lines[blank_at][30:]
            f.write('>%s   contig of %s%s' % (name, g, line_end))
            f.write(line_end.join(lines) + line_end)
    with open(os.path.join(din, g + '.gff'), 'w') as f:
        f.write('##gff-version 3\n\n')
        for c, t, a, b, st, k, _gene in feats:
            fid = 'fig|%s.peg.%d' % (g, k) if k else 'fig|%s.rna.1' % g
            f.write('\t'.join(['accn|' + c, 'PATRIC', t, str(a), str(b), '.', st, '0', 'ID=%s;product=x y' % fid]) + '\n')


def main():
    root = os.path.join(HERE, 'proximal_device')
    if os.path.exists(root):
        shutil.rmtree(root)
    din, dexp = os.path.join(root, 'in'), os.path.join(root, 'expected')
    os.makedirs(din)
    os.makedirs(dexp)
    genomes = {}
    for gi, g in enumerate(MAIN):
        c = base_contigs()
        if g in ('q2', 'q3', 'q4'):               # gene 100: three new variants in each of q2, q3, q4
            for at in (15 + gi, 63 + gi, 130 + gi):
                mutate(c['c2'], at)
            same_window(c['c2'])
        if g in ('q3', 'q4', 'q10'):              # gene 10: its variants first appear in genomes 1, 3 and 4
            mutate(c['c1'], 30)
        if g in ('q4', 'q10'):
            mutate(c['c1'], 33)
        genomes[g] = c
        write_genome(din, g, c, FEATS)
    cx = base_contigs()
    cx['c1'][152] = 'X'                            # inside the upstream window of peg.4 (minus strand)
    write_genome(din, 'qx', cx, FEATS)
    write_genome(din, 'qnc', base_contigs(), FEATS)
    write_genome(din, 'qcr', base_contigs(), FEATS, line_end='\r\n')
    write_genome(din, 'qsp', genomes['q2'], FEATS, blank_at=1)
    names = {}
    for g in MAIN + ['qx', 'qnc', 'qcr', 'qsp']:
        for c, t, a, b, st, k, gene in FEATS:
            if gene is not None:
                names.setdefault(gene, []).append('fig|%s.peg.%d|fam%d' % (g, k, gene))
        if g == 'qnc':
            names.setdefault(9, []).append('fig|qnc.rna.1|fam9')
    with open(os.path.join(din, 'T_allele_names.tsv'), 'w') as f:
        for gene, heads in sorted(names.items()):
            half = (len(heads) + 1) // 2
            f.write('T_C%dA0\t%s\n' % (gene, '\t'.join(heads[:half])))
            if heads[half:]:
                f.write('T_C%dA1\t%s\n' % (gene, '\t'.join(heads[half:])))
    # hand-made extracts (a run that finds them uses them): an empty-sequence record in the middle and one at the end
    pre = os.path.join(din, 'pre')
    os.makedirs(pre)
    foot = '_upstream(-20,3)'
    with open(os.path.join(pre, 'q1_upstream.fna'), 'w') as f:
        f.write('>fig|q1.peg.1%s\nACGTACGT\n>fig|q1.peg.2%s\n\n>fig|q1.peg.3%s\nGGCC\nTTAA\n>fig|q1.peg.7%s\nACGTACGT\n>fig|q1.peg.4%s\n'
                % (foot, foot, foot, foot, foot))
    with open(os.path.join(pre, 'q2_upstream.fna'), 'w') as f:
        f.write('>fig|q2.peg.1%s\nACGTACGT\n>fig|q2.peg.3%s\nGGCCTTAA\n>fig|q2.peg.2%s\n\n' % (foot, foot, foot))

    runs = {}
    for side, limits in (('upstream', UP), ('downstream', DOWN)):
        for mo in (-1, 0, 5):
            runs['%s_mo%d' % (side, mo)] = dict(side=side, genomes=MAIN, kw=dict(limits=limits, max_overlap=mo), host=[])
    runs['upstream_mo5_frag'] = dict(side='upstream', genomes=MAIN, kw=dict(limits=UP, max_overlap=5, include_fragments=True,
                                                                            fna_output_footer='_f', name='F'), host=[])
    runs['downstream_mo-1_frag'] = dict(side='downstream', genomes=MAIN, kw=dict(limits=DOWN, include_fragments=True), host=[])
    runs['bad_base'] = dict(side='upstream', genomes=['q1', 'qx', 'q2'], kw=dict(limits=UP), host=['qx'])
    runs['noncds_mo-1'] = dict(side='upstream', genomes=['q1', 'qnc'], kw=dict(limits=UP), host=[])
    runs['noncds_mo0'] = dict(side='upstream', genomes=['q1', 'qnc', 'q2'], kw=dict(limits=UP, max_overlap=0), host=['qnc'])
    runs['odd_files'] = dict(side='downstream', genomes=['qcr', 'q3', 'qsp'], kw=dict(limits=DOWN, max_overlap=5), host=['qcr', 'qsp'])
    runs['preexisting'] = dict(side='upstream', genomes=['q1', 'q2', 'q3'], kw=dict(limits=UP), host=[], pre=['q1', 'q2'])
    for tag, r in runs.items():
        out = os.path.join(dexp, tag)
        os.makedirs(out)
        derived = os.path.join(din, 'derived')
        os.makedirs(derived)
        for g in r.get('pre', []):
            shutil.copy(os.path.join(pre, '%s_%s.fna' % (g, r['side'])), derived)
        fn = ref_pg.build_upstream_pangenome if r['side'] == 'upstream' else ref_pg.build_downstream_pangenome
        pairs = [(os.path.join(din, g + '.gff'), os.path.join(din, g + '.fna')) for g in r['genomes']]
        buf, r['raised'] = io.StringIO(), None
        with contextlib.redirect_stdout(buf):
            try:
                fn(pairs, os.path.join(din, 'T_allele_names.tsv'), out, **r['kw'])
            except Exception as e:                # noqa: BLE001 -- whatever the reference raises is the record
                r['raised'] = [type(e).__name__, [str(a) for a in e.args]]
        r['stdout'] = buf.getvalue().replace(din, '<in>').replace(out, '<out>')
        r['kw']['limits'] = list(r['kw']['limits'])
        for f in sorted(os.listdir(derived)):     # the per-genome extracts land next to the inputs: move them
            shutil.move(os.path.join(derived, f), os.path.join(out, f))
        shutil.rmtree(derived)
        r['files'] = sorted(os.listdir(out))
    json.dump(runs, open(os.path.join(dexp, 'runs.json'), 'w'), indent=0, sort_keys=True)

    # what the fixtures are there for
    def text(tag, name):
        return open(os.path.join(dexp, tag, name)).read()
    for side in ('upstream', 'downstream'):
        a, b, c = (text('%s_mo%d' % (side, mo), 'q1_%s.fna' % side) for mo in (-1, 0, 5))
        strip = lambda s: [x for x in s.split('\n') if not x.startswith('>')]      # noqa: E731
        assert strip(a) != strip(b) and strip(b) != strip(c) and strip(a) != strip(c), side     # truncations on this side
        labels = text('%s_mo-1' % side, 'Test_strain_by_%s.npz.labels.txt' % side).split('\n')
        letter = side[0].upper()
        assert labels.index('T_C100%s0' % letter) < labels.index('T_C10%s0' % letter) < labels.index('T_C2%s0' % letter), labels
    labels = text('upstream_mo-1', 'Test_strain_by_upstream.npz.labels.txt').split('\n')
    assert labels.index('T_C100U10') < labels.index('T_C100U11') < labels.index('T_C100U2'), labels
    labels = text('downstream_mo-1', 'Test_strain_by_downstream.npz.labels.txt').split('\n')
    assert labels.index('T_C100D0') < labels.index('T_C10D0') < labels.index('T_C1D0') < labels.index('T_C2D0'), labels
    nr = text('upstream_mo-1', 'Test_nr_upstream.fna').split('\n')
    seq_of = dict(zip((x[1:] for x in nr[0::2]), nr[1::2]))
    assert seq_of['T_C6U0'] in [v for k, v in seq_of.items() if k.startswith('T_C100U')]        # one window, two genes
    assert 'T_C10U2' in text('upstream_mo-1', 'Test_strain_by_upstream.npz.labels.txt')
    assert text('upstream_mo5_frag', 'q1_upstream_f.fna') != text('upstream_mo5', 'q1_upstream.fna')
    assert 'peg.11_' in text('upstream_mo5_frag', 'q1_upstream_f.fna') and 'peg.11_' not in text('upstream_mo5', 'q1_upstream.fna')
    assert any(ch in text('upstream_mo-1', 'q1_upstream.fna') for ch in 'nN') and any(ch in text('upstream_mo-1', 'q1_upstream.fna') for ch in 'ry')
    assert runs['bad_base']['raised'] == ['KeyError', ['X']] and runs['noncds_mo0']['raised'][0] == 'KeyError'
    assert runs['noncds_mo-1']['raised'] is None and runs['odd_files']['raised'] is None and runs['preexisting']['raised'] is None
    assert 'qx_upstream.fna' in runs['bad_base']['files'] and 'q2_upstream.fna' not in runs['bad_base']['files']
    assert 'rna.1' in text('noncds_mo-1', 'qnc_upstream.fna')
    size = sum(os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(root) for f in fs)
    print('proximal_device: %d runs, %d bytes' % (len(runs), size))


if __name__ == '__main__':
    main()
