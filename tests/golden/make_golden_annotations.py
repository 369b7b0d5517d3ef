"""Writes tests/golden/annotations: what the reference's extract_annotations and generate_annotations (pangenome.py:1650-1810)
wrote, printed, returned and raised on inputs of a few lines each. Needs the reference checkout: its directory is the first
argument or $PANGENOMIX_REFERENCE (imported as tests/golden/make_golden_next.py does); nothing of it is copied. The
reference calls urllib.unquote, which Python 3 does not have (AttributeError on the first line with ID and product), so
ref_pg.urllib.unquote is bound to urllib.parse.unquote here, at run time; its file is untouched.

Layout: <case>/ holds the inputs (GFFs, names.tsv or annotation files) and expected.tsv where a file was written; cases.json
holds per case the arguments, whether the device path must take it (`regular`), stdout, and the exception's type and
argument. A case is regular unless it says why not."""
import contextlib
import io
import json
import os
import shutil
import sys
import types
import urllib.parse

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else os.environ['PANGENOMIX_REFERENCE']
sys.path.insert(0, REFERENCE)
sys.path.insert(0, os.path.join(REFERENCE, 'pangenomix'))
for _name in ('statsmodels', 'statsmodels.stats', 'Bio', 'Bio.SeqIO'):
    sys.modules.setdefault(_name, types.ModuleType(_name))
sys.modules['statsmodels'].stats = sys.modules['statsmodels.stats']
sys.modules['Bio'].SeqIO = sys.modules['Bio.SeqIO']

import pangenomix.pangenome as ref_pg                     # noqa: E402

ref_pg.urllib.unquote = urllib.parse.unquote

OUT = os.path.join(HERE, 'annotations')


def gff(records, head='##gff-version 3\n', eol='\n'):
    """records: (type, attributes) -> a GFF file; coordinates do not matter here"""
    lines = ['acc|c1\tPATRIC\t%s\t%d\t%d\t.\t+\t0\t%s' % (ty, 10 + 100 * i, 90 + 100 * i, attrs)
             for i, (ty, attrs) in enumerate(records)]
    return head + ''.join(line + eol for line in lines)


G1 = gff([('CDS', 'ID=fig|1.1.peg.1;locus_tag=L1_1;product=thr operon leader peptide'),
          ('CDS', 'ID=fig|1.1.peg.2;locus_tag=L1_2;product=Aspartokinase%20%28EC%202.7.2.4%29'),
          ('CDS', 'ID=fig|1.1.peg.3;product=hypothetical protein'),
          ('tRNA', 'ID=fig|1.1.rna.1;product=tRNA-Ala'),
          ('CDS', 'ID=fig|1.1.peg.4;locus_tag=L1_4;product=Transporter%2C MFS;note=x'),
          ('CDS', 'ID=fig|1.1.peg.5;locus_tag=L1_5'),                                  # no product: not a record
          ('CDS', 'ID=fig|1.1.peg.6;locus_tag=L1_6;product=first;product=Kinase;ID=fig|1.1.peg.7')])   # later entries win
G2 = gff([('CDS', 'ID=fig|2.1.peg.1;locus_tag=L2_1;product=thr operon leader peptide'),
          ('CDS', 'ID=fig|2.1.peg.2;locus_tag=L2_2;product=Aspartokinase (EC 2.7.2.4)'),
          ('CDS', 'ID=fig|2.1.peg.3;product=Phage protein'),
          ('tRNA', 'ID=fig|2.1.rna.1;locus_tag=L2_r1;product=tRNA-Ala'),
          ('CDS', 'ID=fig|2.1.peg.4;locus_tag=L2_4;product=Transporter, MFS'),
          ('CDS', 'ID=fig|2.1.peg.4;locus_tag=L2_4;product=Transporter, ABC')], head='')   # the same key twice in a file
NAMES = '\n'.join(['T_C0A0\tfig|1.1.peg.1|L1_1\tfig|2.1.peg.1|L2_1',               # two ids of a row with one product
                   'T_C0A1\tfig|9.9.peg.1|X',                                        # an id nothing maps
                   'T_C1A0\tfig|1.1.peg.2|L1_2',
                   'T_C1A1\tfig|2.1.peg.2|L2_2',                                     # the same product, percent-encoded in g1
                   'T_C1A2\tfig|2.1.peg.3',
                   'T_C2A0\tfig|1.1.peg.3\tfig|2.1.peg.3',
                   'T_C2A1\tfig|2.1.peg.3\tfig|1.1.peg.3',                           # the same set in another order: a tie,
                   'T_C2A2',                                                         # ... a row with no id
                   'T_C3A0\tfig|1.1.peg.4|L1_4\tfig|2.1.peg.4|L2_4',
                   'T_C3A1\tfig|1.1.peg.7|L1_6\tfig|1.1.rna.1\tfig|2.1.rna.1|L2_r1\tfig|2.1.rna.1',
                   'T_C0A2\tfig|1.1.peg.1|L1_1',                                     # gene C0 comes back
                   'T_T4A0\tfig|1.1.rna.1',
                   'last_C5A0\tfig|1.1.peg.5|L1_5']) + '\n'                           # the last gene: never written
TIE = '\n'.join(['T_C0A0\tfig|2.1.peg.3', 'T_C0A1\tfig|1.1.peg.3', 'T_C0A2\tfig|1.1.peg.3', 'T_C0A3\tfig|2.1.peg.3',
                 'T_C0A4\tunmapped', 'T_C1A0\tfig|1.1.peg.3']) + '\n'
NO_A = '\n'.join(['x1\tfig|1.1.peg.3', 'x2\tfig|2.1.peg.3', 'y3\tfig|1.1.peg.3', 'T_C1A0\tfig|1.1.peg.3', 'z\tq']) + '\n'
# the same key in two files with different products
K1 = gff([('CDS', 'ID=k;locus_tag=t;product=from one'), ('CDS', 'ID=only1;product=one')])
K2 = gff([('CDS', 'ID=k;locus_tag=t;product=from two'), ('CDS', 'ID=only2;product=two')])
KN = 'T_C0A0\tk|t\nT_C0A1\tonly1\tonly2\nT_C1A0\tk|t\n'
# a product that is a key of a later file
P1 = gff([('CDS', 'ID=a;product=b')])
P2 = gff([('CDS', 'ID=b;product=Z')])
PN = 'T_C0A0\ta\nT_C0A1\tb\nT_C1A0\ta\n'

EXTRACT = {
    # case: (gffs {name: text}, names text, kwargs, why the device path leaves it to the host or None)
    'two_gffs_batch100': ({'g1.gff': G1, 'g2.gff': G2}, NAMES, dict(batch=100), None),
    'two_gffs_batch1': ({'g1.gff': G1, 'g2.gff': G2}, NAMES, dict(batch=1), None),
    'collapse_false': ({'g1.gff': G1, 'g2.gff': G2}, NAMES, dict(collapse_alleles=False), None),
    'flexible_locus_tag': ({'g1.gff': G1, 'g2.gff': G2}, NAMES, dict(flexible_locus_tag=True), None),
    'allowed_trna': ({'g1.gff': G1, 'g2.gff': G2}, NAMES, dict(allowed_features=['tRNA'], flexible_locus_tag=True), None),
    'tie_first_seen': ({'g1.gff': G1, 'g2.gff': G2}, TIE, dict(), None),
    'single_gene': ({'g1.gff': G1}, 'T_C0A0\tfig|1.1.peg.3\nT_C0A1\tfig|1.1.peg.1|L1_1\n', dict(), None),
    'alleles_without_a': ({'g1.gff': G1, 'g2.gff': G2}, NO_A, dict(), None),
    'same_key_batch100': ({'k1.gff': K1, 'k2.gff': K2}, KN, dict(batch=100), None),
    'same_key_batch1': ({'k1.gff': K1, 'k2.gff': K2}, KN, dict(batch=1), None),
    'no_gffs': ({}, NAMES, dict(), None),
    'tab_in_product': ({'g.gff': gff([('CDS', 'ID=a;product=two%09tokens'), ('CDS', 'ID=b;product=two'),
                                      ('CDS', 'ID=c;product=tokens')])},
                       'T_C0A0\ta\nT_C0A1\tb\tc\nT_C0A2\tb\nT_C1A0\ta\n', dict(), 'a decoded product holds a tab'),
    'product_is_later_key_batch100': ({'p1.gff': P1, 'p2.gff': P2}, PN, dict(batch=100), 'a product equals a key'),
    'product_is_later_key_batch1': ({'p1.gff': P1, 'p2.gff': P2}, PN, dict(batch=1), 'a product equals a key'),
    'attribute_without_equals': ({'g.gff': gff([('CDS', 'ID=a;product=x'), ('CDS', 'ID=b;flag;product=y')])},
                                 'T_C0A0\ta\nT_C1A0\tb\n', dict(), 'an attribute entry without ='),
    'attribute_with_two_equals': ({'g.gff': gff([('CDS', 'ID=a;product=x'), ('CDS', 'ID=b;product=y=z')])},
                                  'T_C0A0\ta\nT_C1A0\tb\n', dict(), 'an attribute entry with two ='),
    'blank_names_line': ({'g1.gff': G1}, 'T_C0A0\tfig|1.1.peg.3\n\nT_C0A1\tfig|1.1.peg.3\nT_C1A0\tx\n', dict(),
                         'a blank names line'),
    'crlf': ({'g1.gff': gff([('CDS', 'ID=a;product=x y'), ('CDS', 'ID=b;locus_tag=t;product=z')], eol='\r\n')},
             'T_C0A0\ta\r\nT_C0A1\tb|t\r\nT_C1A0\ta\r\n', dict(), 'CRLF line ends'),
    'non_ascii_product': ({'g.gff': gff([('CDS', 'ID=a;product=caf%C3%A9%FF'), ('CDS', 'ID=b;product=plain')])},
                          'T_C0A0\ta\nT_C0A1\tb\nT_C1A0\ta\n', dict(), 'a product that is not ASCII once decoded'),
    'empty_product': ({'g.gff': gff([('CDS', 'ID=a;product='), ('CDS', 'ID=b;product=plain')])},
                      'T_C0A0\ta\tb\nT_C0A1\tb\nT_C1A0\ta\n', dict(), 'an empty product'),
}

A1 = 'T_C0\tthr operon leader peptide\nT_C0A1\tfig|9.9.peg.1|X\nT_C1\tAspartokinase (EC 2.7.2.4)\tsecond\nT_T4\ttRNA-Ala\n'
A2 = 'T_C1\tfrom the later file\nT_C7\nT_C0A1\tlater line\n'
GENERATE = {
    # case: (annotation files {name: text}, features, why the device path leaves it to the host or None)
    'own_and_cluster': ({'a1.tsv': A1}, ['T_C0', 'T_C0A1', 'T_C0A0', 'T_C1A5', 'T_T4A0'], None),
    'utr_variants': ({'a1.tsv': A1}, ['T_C0U3', 'T_C1D0', 'T_T4U1'], None),
    'missing_is_nan': ({'a1.tsv': A1}, ['T_C9', 'T_C9A0', 'T_C0'], None),
    'all_missing': ({'a1.tsv': A1}, ['T_C9', 'T_C8A0'], None),
    'duplicate_features': ({'a1.tsv': A1}, ['T_C0', 'T_C1A0', 'T_C0', 'T_C1A0'], None),
    'later_file_wins': ({'a1.tsv': A1, 'a2.tsv': A2}, ['T_C1', 'T_C1A0', 'T_C0A1', 'T_C7', 'T_C7A2', 'T_C0'], None),
    'unreadable_name': ({'a1.tsv': A1}, ['T_C0', 'nonsense', 'T_C1'], 'breakdown_feature_name raises'),
}


@contextlib.contextmanager
def recorded(record):
    buf = io.StringIO()
    record['exception'] = None
    try:
        with contextlib.redirect_stdout(buf):
            yield
    except Exception as e:                                   # noqa: BLE001 -- whatever the reference raises is the record
        record['exception'] = [type(e).__name__, str(e.args[0]) if e.args else '']
    record['stdout'] = buf.getvalue()


def write_inputs(case, files):
    d = os.path.join(OUT, case)
    os.makedirs(d)
    for name, text in files.items():
        with open(os.path.join(d, name), 'w', newline='') as f:
            f.write(text)
    return d


def main():
    if os.path.isdir(OUT):
        shutil.rmtree(OUT)
    os.makedirs(OUT)
    cases = {'extract': {}, 'generate': {}}
    for case, (gffs, names, kwargs, why) in EXTRACT.items():
        d = write_inputs(case, dict(gffs, **{'names.tsv': names}))
        out = os.path.join(d, 'expected.tsv')
        record = dict(gffs=list(gffs), kwargs=kwargs, regular=why is None, why=why)
        with recorded(record):
            ref_pg.extract_annotations([os.path.join(d, g) for g in gffs], os.path.join(d, 'names.tsv'), out, **kwargs)
        record['output'] = os.path.exists(out)
        record['tmp_left'] = sorted(f for f in os.listdir(d) if '.tmp' in f)
        for f in record['tmp_left']:
            os.remove(os.path.join(d, f))
        if record['exception'] is not None and record['output']:
            os.remove(out)                                   # (a partial file: what it holds depends on buffering)
            record['output'] = False
        cases['extract'][case] = record
    for case, (files, features, why) in GENERATE.items():
        d = write_inputs(case, files)
        record = dict(files=list(files), features=features, regular=why is None, why=why, expected=None, dtype=None)
        with recorded(record):
            series = ref_pg.generate_annotations(features, [os.path.join(d, f) for f in files])
            assert list(series.index) == features
            record['expected'] = [None if isinstance(v, float) and np.isnan(v) else v for v in series.tolist()]
            record['dtype'] = str(series.dtype)
        cases['generate'][case] = record
    with open(os.path.join(OUT, 'cases.json'), 'w') as f:
        json.dump(cases, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    main()
