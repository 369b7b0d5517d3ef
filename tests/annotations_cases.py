"""TEST INFRASTRUCTURE shared by test_annotations_host.py and test_gpu_annotations.py: the cases the reference recorded
(tests/golden/annotations, written by tests/golden/make_golden_annotations.py), run through pangenomix_amd.pangenome with or
without a context and reduced to one comparable record, and a generated set that is larger than a fixture should be."""
import json
import math
import os
import shutil

import numpy as np

from pangenomix_amd import pangenome as pg

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'annotations')
CASES = json.load(open(os.path.join(GOLDEN, 'cases.json')))
EXTRACT_CASES = sorted(CASES['extract'])
GENERATE_CASES = sorted(CASES['generate'])


def load_case(case):
    return CASES['extract'][case] if case in CASES['extract'] else CASES['generate'][case]


def _exception(e):
    return [type(e).__name__, str(e.args[0]) if e.args else '']


def run_extract(case, workdir, capsys, ctx):
    """{'stdout', 'exception', 'output' (the file's bytes or None), 'tmp_left'} of one recorded case on a copy of its inputs"""
    record = CASES['extract'][case]
    shutil.copytree(os.path.join(GOLDEN, case), str(workdir))
    expected = os.path.join(str(workdir), 'expected.tsv')
    if os.path.exists(expected):
        os.remove(expected)
    out = os.path.join(str(workdir), 'out.tsv')
    capsys.readouterr()
    got = dict(exception=None)
    try:
        pg.extract_annotations([os.path.join(str(workdir), g) for g in record['gffs']], os.path.join(str(workdir), 'names.tsv'),
                               out, ctx=ctx, **record['kwargs'])
    except Exception as e:                                   # noqa: BLE001 -- compared with the reference's
        got['exception'] = _exception(e)
    got['stdout'] = capsys.readouterr().out
    got['tmp_left'] = sorted(f.replace('out.tsv', 'expected.tsv') for f in os.listdir(str(workdir)) if '.tmp' in f)
    got['output'] = open(out, 'rb').read() if got['exception'] is None and os.path.exists(out) else None
    return got


def run_generate(case, workdir, ctx):
    """{'exception', 'expected' (None for NaN), 'dtype'} of one recorded case"""
    record = CASES['generate'][case]
    got = dict(exception=None, expected=None, dtype=None)
    try:
        series = pg.generate_annotations(record['features'], [os.path.join(GOLDEN, case, f) for f in record['files']], ctx=ctx)
        assert list(series.index) == record['features']
        got['expected'] = [None if isinstance(v, float) and math.isnan(v) else v for v in series.tolist()]
        got['dtype'] = str(series.dtype)
    except Exception as e:                                   # noqa: BLE001
        got['exception'] = _exception(e)
    return got


def assert_recorded(case, got):
    """what pangenomix_amd gave against what the reference gave"""
    record = load_case(case)
    assert got['exception'] == record['exception']
    if case in CASES['generate']:
        assert got['expected'] == record['expected'] and got['dtype'] == record['dtype']
        return
    assert got['stdout'] == record['stdout']
    assert got['tmp_left'] == record['tmp_left']
    if record['output']:
        assert got['output'] == open(os.path.join(GOLDEN, case, 'expected.tsv'), 'rb').read()
    else:
        assert got['output'] is None


PRODUCTS = ['hypothetical protein', 'Transporter%2C MFS family', 'DNA-directed RNA polymerase beta%27 subunit %28EC 2.7.7.6%29',
            'tRNA-Ala', 'Mobile element protein', '50S ribosomal protein L7%2FL12', 'Phage tail fiber', 'ABC transporter%2C ATP-binding']


def generated_set(workdir, n_genomes, n_genes, big_run, big_row, seed=5):
    """(GFF paths, names path): every genome holds one CDS per gene; a gene has one allele per distinct product variant and
    an allele lists the genomes that carry it. Gene 7 has `big_run` alleles, allele 0 of gene 11 lists `big_row` ids (extra
    records of genome 0). Products come from a few strings, some percent-encoded, one in eight ids has no locus_tag."""
    rng = np.random.default_rng(seed)
    records = [[] for _ in range(n_genomes)]                 # per genome: (id, locus_tag or None, product)
    lines = []
    for gene in range(n_genes):
        n_alleles = big_run if gene == 7 else int(rng.integers(1, 5))
        base = int(rng.integers(0, len(PRODUCTS)))
        for allele in range(n_alleles):
            carriers = [int(rng.integers(0, n_genomes))] if allele else list(range(n_genomes))
            copies = big_row if (gene == 11 and allele == 0) else 1
            fids = []
            for genome in carriers:
                for copy in range(copies if genome == 0 else 1):
                    peg = 'fig|%d.1.peg.%d' % (genome + 1, len(records[genome]) + 1)
                    tag = None if rng.integers(0, 8) == 0 else 'L%d_%d' % (genome + 1, len(records[genome]) + 1)
                    odd = rng.integers(0, 6) == 0            # now and then another product: alleles that differ, and ties
                    product = PRODUCTS[(base + (1 + copy % 3 if odd else 0)) % len(PRODUCTS)]
                    records[genome].append((peg, tag, product))
                    fids.append(peg if tag is None else peg + '|' + tag)
            if rng.integers(0, 25) == 0:
                fids.append('fig|0.0.peg.%d' % gene)         # an id no GFF holds
            lines.append('\t'.join(['G_C%dA%d' % (gene, allele)] + fids))
    gffs = []
    for genome, recs in enumerate(records):
        path = os.path.join(str(workdir), 'genome%d.gff' % genome)
        with open(path, 'w') as f:
            f.write('##gff-version 3\n')
            for i, (peg, tag, product) in enumerate(recs):
                attrs = 'ID=%s;%sproduct=%s' % (peg, '' if tag is None else 'locus_tag=%s;' % tag, product)
                f.write('acc|c1\tPATRIC\tCDS\t%d\t%d\t.\t+\t0\t%s\n' % (1 + 100 * i, 90 + 100 * i, attrs))
        gffs.append(path)
    names = os.path.join(str(workdir), 'G_allele_names.tsv')
    with open(names, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    return gffs, names
