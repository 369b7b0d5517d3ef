"""Novel-allele calls (`~n`) of pangenomix_amd.mlst on the host path (ctx=None; call_alleles(min_identity=...), run_mlst(minid=...))
against the hand-written fixtures tests/golden/mlst_novel (its README says what each genome carries and why) and
tests/golden/mlst, and the fixtures themselves against the brute-force model of the bounded-mismatch scan."""
import os

import numpy as np
import pandas as pd
import pytest

import near_scan_model as model
import test_mlst_host as exact
from pangenomix_amd import mlst, pangenome_analysis as pa

G6_NOVEL = ('g6.fna', 'abcA', 1, 'g6_contig1', 51, '+', 0, 1)


def fixture(golden_dir):
    root = os.path.join(golden_dir, 'mlst_novel')
    genomes = [os.path.join(root, 'genomes', 'n%d.fna' % i) for i in range(1, 5)]
    return root, os.path.join(golden_dir, 'mlst', 'scheme'), genomes


def expected_lines(root):
    with open(os.path.join(root, 'expected_mlst.tsv')) as f:
        return ''.join(os.path.join(root, 'genomes', line) for line in f)


def expected_hits(root):
    hits = pd.read_csv(os.path.join(root, 'expected_hits.tsv'), sep='\t')
    hits['genome'] = [os.path.join(root, 'genomes', g) for g in hits['genome']]
    return hits


def old_fixture_expectations(golden_dir):
    """tests/golden/mlst at 95 %: g1-g5 keep their lines and hits, g6 becomes abcA(~1) with one hit row in front of ghiC's"""
    root, scheme_dir, genomes = exact.fixture(golden_dir)
    lines = exact.expected_lines(root).replace('abcA(-)\tdefB(-)\tghiC(4)', 'abcA(~1)\tdefB(-)\tghiC(4)')
    assert lines != exact.expected_lines(root)
    hits = exact.expected_hits(root)
    hits['mismatches'] = 0
    row = pd.DataFrame([(os.path.join(root, 'genomes', G6_NOVEL[0]),) + G6_NOVEL[1:]], columns=mlst.NEAR_HIT_COLUMNS)
    hits = pd.concat([hits.iloc[:-1], row, hits.iloc[-1:]], ignore_index=True)
    return root, scheme_dir, genomes, lines, hits


def lines_of(frame, scheme):
    return ''.join(mlst.format_mlst_line(r[0], r[1], r[2], scheme.loci, r[3:]) + '\n' for r in frame.itertuples(index=False))


def assert_hits_equal(hits, want):
    assert list(hits.columns) == mlst.NEAR_HIT_COLUMNS == list(want.columns)
    assert hits.astype(str).values.tolist() == want.astype(str).values.tolist()


def test_novel_fixture_calls_and_hits_equal_the_recorded_files(golden_dir, tmp_path):
    root, scheme_dir, genomes = fixture(golden_dir)
    scheme = mlst.load_scheme(scheme_dir)
    mlst.MLST_PATH_COUNTS.clear()
    frame, hits = mlst.call_alleles(scheme, genomes, return_hits=True, min_identity=95)
    assert mlst.MLST_PATH_COUNTS == {'host': 4}
    assert lines_of(frame, scheme) == expected_lines(root)
    assert_hits_equal(hits, expected_hits(root))
    assert mlst.call_alleles(scheme, genomes, min_identity=95).equals(frame)
    out = pa.run_mlst(genomes, str(tmp_path / 'out.tsv'), scheme_dir=scheme_dir, minid=95)
    assert out.equals(frame) and open(tmp_path / 'out.tsv').read() == expected_lines(root)
    # without the argument the same genomes have no call where the allele is novel
    plain = mlst.call_alleles(scheme, genomes)
    assert ['-' if '~' in c else c for c in frame.iloc[:, 3:].values.ravel()] == plain.iloc[:, 3:].values.ravel().tolist()


def test_exact_fixture_at_95_percent(golden_dir, tmp_path):
    root, scheme_dir, genomes, lines, want_hits = old_fixture_expectations(golden_dir)
    scheme = mlst.load_scheme(scheme_dir)
    frame, hits = mlst.call_alleles(scheme, genomes, return_hits=True, min_identity=95)
    assert lines_of(frame, scheme) == lines
    assert_hits_equal(hits, want_hits)
    assert frame['ST'].tolist() == ['1', '2', '-', '4', '-', '-']
    pa.run_mlst(os.path.join(root, 'genomes'), str(tmp_path / 'out.tsv'), scheme_dir=scheme_dir, minid=95)
    assert open(tmp_path / 'out.tsv').read() == lines


def revcomp(seq):
    return seq.translate(bytes.maketrans(b'ACGTWSRYMKN', b'TGCAWSYRKMN'))[::-1]


def brute_force_calls(scheme, path, min_identity):
    """The rules of call_alleles' docstring on the model alone: exact calls by `in`, else every allele on both strands against
    every window of the genome. Returns the calls of the loci."""
    _, contigs = mlst.read_genome(path)
    text = b'\x00'.join(contigs)
    calls = []
    for locus in scheme.loci:
        alleles = [(number, seq.upper()) for number, seq in scheme.alleles[locus]]
        found = [(n, s) for n, s in alleles if s in text or revcomp(s) in text]
        kept = sorted(n for n, s in found if not any(len(t) > len(s) and s in t for _, t in found))
        if kept:
            calls.append(','.join(str(n) for n in kept))
            continue
        patterns = [s for _, s in alleles] + [revcomp(s) for _, s in alleles]
        mm = [len(p) * (10000 - int(round(min_identity * 100))) // 10000 for p in patterns]
        best = model.best(text, patterns, mm, separator=0)
        ranked = []
        for i, (number, seq) in enumerate(alleles):
            hit = min(int(best[i]), int(best[len(alleles) + i]))
            if hit != model.NONE:
                ranked.append((hit >> 32, -len(seq), number))
        calls.append('~%d' % min(ranked)[2] if ranked else '-')
    return calls


def test_the_brute_force_model_reproduces_every_expected_call(golden_dir):
    root, scheme_dir, genomes = fixture(golden_dir)
    scheme = mlst.load_scheme(scheme_dir)
    want = [line.rstrip('\n').split('\t') for line in open(os.path.join(root, 'expected_mlst.tsv'))]
    for path, cells in zip(genomes, want):
        assert os.path.basename(path) == cells[0]
        assert ['%s(%s)' % lc for lc in zip(scheme.loci, brute_force_calls(scheme, path, 95))] == cells[3:]
    root, _, genomes, lines, _ = old_fixture_expectations(golden_dir)
    for path, line in zip(genomes, lines.splitlines()):
        assert ['%s(%s)' % lc for lc in zip(scheme.loci, brute_force_calls(scheme, path, 95))] == line.split('\t')[3:]
    # the hit rows of the novel calls: the model's best window of the called allele, on the recorded strand
    hits = expected_hits(fixture(golden_dir)[0])
    for row in hits[hits['copies'] == 0].itertuples(index=False):
        names, contigs = mlst.read_genome(row.genome)
        seq = dict(scheme.alleles[row.locus])[row.allele].upper()
        pattern = seq if row.strand == '+' else revcomp(seq)
        contig = contigs[names.index(row.contig)]
        d, at = model.distance_and_position(model.best(contig, [pattern], [len(pattern)])[0])
        assert (d, at + 1) == (row.mismatches, row.start), row


def test_without_min_identity_nothing_changes(golden_dir):
    root, scheme_dir, genomes = exact.fixture(golden_dir)
    scheme = mlst.load_scheme(scheme_dir)
    frame, hits = mlst.call_alleles(scheme, genomes, return_hits=True, min_identity=None)
    old_frame, old_hits = mlst.call_alleles(scheme, genomes, return_hits=True)
    assert frame.equals(old_frame) and hits.equals(old_hits)
    exact.assert_frame_as_recorded(frame, scheme, root)
    exact.assert_hits_as_recorded(hits, root)


def test_at_100_percent_nothing_novel_is_called(golden_dir):
    for root, scheme_dir, genomes in (exact.fixture(golden_dir), fixture(golden_dir)):
        scheme = mlst.load_scheme(scheme_dir)
        frame, hits = mlst.call_alleles(scheme, genomes, return_hits=True, min_identity=100)
        plain, plain_hits = mlst.call_alleles(scheme, genomes, return_hits=True)
        assert frame.equals(plain) and not frame.astype(str).apply(lambda c: c.str.contains('~')).values.any()
        assert hits[mlst.HIT_COLUMNS].equals(plain_hits) and (hits['mismatches'] == 0).all()


def test_threshold_formula():
    m = mlst.max_mismatches
    assert [m(L, 95) for L in (19, 20, 40, 59, 60, 450, 5120)] == [0, 1, 2, 2, 3, 22, 256]
    assert [m(L, 99.5) for L in (199, 200, 450, 1000)] == [0, 1, 2, 5]
    assert [m(L, 100) for L in (1, 450, 100000)] == [0, 0, 0]
    assert m(450, 95.0) == m(450, 95) and m(1000, 90) == 100 and m(3, 0.01) == 2
    for bad in (0, -5, 100.5):
        with pytest.raises(ValueError):
            m(450, bad)
    with pytest.raises(ValueError):
        mlst.call_alleles(mlst.Scheme('s', ['x'], {'x': [(1, b'ACGT')]}, {}), [], min_identity=0)


def test_a_scheme_with_a_short_block_and_a_wide_budget(tmp_path):
    """30 bases at 80 %: m = 6, blocks of 4 bases; six substitutions are called, seven are not, on either strand"""
    rng = np.random.default_rng(3)
    letters = np.frombuffer(b'ACGT', dtype=np.uint8)
    allele = letters[rng.integers(0, 4, 30)].tobytes()
    scheme = mlst.Scheme('s', ['x'], {'x': [(1, allele)]}, {(1,): '1'})
    assert mlst.max_mismatches(30, 80) == 6
    paths = []
    for name, places, reverse in (('six', (0, 5, 9, 14, 18, 22), False), ('seven', (0, 5, 9, 14, 18, 22, 27), False),
                                  ('six_rc', (1, 6, 10, 15, 19, 23), True)):
        seq = model.mutate(allele, places).replace(b'\x14', b'N').replace(b'\x16', b'N').replace(b'\x12', b'N').replace(b'\x01', b'N')
        filler = letters[rng.integers(0, 4, 400)].tobytes()
        paths.append(str(tmp_path / (name + '.fna')))
        with open(paths[-1], 'wb') as f:
            f.write(b'>c\n' + filler[:170] + (revcomp(seq) if reverse else seq) + filler[170:] + b'\n')
    frame, hits = mlst.call_alleles(scheme, paths, return_hits=True, min_identity=80)
    assert frame['x'].tolist() == ['~1', '-', '~1'] and frame['ST'].tolist() == ['-', '-', '-']
    assert hits[['start', 'strand', 'copies', 'mismatches']].values.tolist() == [[171, '+', 0, 6], [171, '-', 0, 6]]
    assert [brute_force_calls(scheme, p, 80) for p in paths] == [['~1'], ['-'], ['~1']]
