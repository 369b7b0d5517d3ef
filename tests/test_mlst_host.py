"""pangenomix_amd.mlst on the host path (ctx=None), and pangenome_analysis.run_mlst, against the hand-written fixture
tests/golden/mlst (its README says what each genome carries and why), plus the errors of load_scheme."""
import os
import shutil

import numpy as np
import pandas as pd
import pytest

from pangenomix_amd import mlst, pangenome_analysis as pa, synth


def fixture(golden_dir):
    root = os.path.join(golden_dir, 'mlst')
    genomes = [os.path.join(root, 'genomes', 'g%d.fna' % i) for i in range(1, 7)]
    return root, os.path.join(root, 'scheme'), genomes


def expected_lines(root):
    """the recorded output with the genomes' directory in front of every file name"""
    with open(os.path.join(root, 'expected_mlst.tsv')) as f:
        return ''.join(os.path.join(root, 'genomes', line) for line in f)


def expected_hits(root):
    hits = pd.read_csv(os.path.join(root, 'expected_hits.tsv'), sep='\t')
    hits['genome'] = [os.path.join(root, 'genomes', g) for g in hits['genome']]
    return hits


def assert_frame_as_recorded(frame, scheme, root):
    lines = ''.join(mlst.format_mlst_line(r[0], r[1], r[2], scheme.loci, r[3:]) + '\n' for r in frame.itertuples(index=False))
    assert lines == expected_lines(root)


def assert_hits_as_recorded(hits, root):
    want = expected_hits(root)
    assert list(hits.columns) == mlst.HIT_COLUMNS == list(want.columns)
    assert hits.astype(str).values.tolist() == want.astype(str).values.tolist()


def test_load_scheme(golden_dir):
    root, scheme_dir, _ = fixture(golden_dir)
    scheme = mlst.load_scheme(scheme_dir)
    assert scheme.name == 'demo' and scheme.loci == ['abcA', 'defB', 'ghiC']               # the metadata columns are no loci
    assert [n for n, _ in scheme.alleles['defB']] == [1, 2, 3, 4, 5] and len(scheme.alleles['abcA']) == 4
    assert all(40 <= len(s) <= 60 for records in scheme.alleles.values() for _, s in records)
    assert scheme.profiles == {(1, 1, 1): '1', (2, 1, 3): '2', (3, 3, 1): '3', (4, 2, 2): '4', (1, 4, 1): '5'}
    assert mlst.load_scheme(scheme_dir, 'demo') == scheme


def test_calls_and_hits_equal_the_recorded_files(golden_dir):
    root, scheme_dir, genomes = fixture(golden_dir)
    scheme = mlst.load_scheme(scheme_dir)
    mlst.MLST_PATH_COUNTS.clear()
    frame, hits = mlst.call_alleles(scheme, genomes, return_hits=True)
    assert mlst.MLST_PATH_COUNTS == {'host': 6}
    assert list(frame.columns) == ['genome', 'scheme', 'ST', 'abcA', 'defB', 'ghiC']
    assert_frame_as_recorded(frame, scheme, root)
    assert_hits_as_recorded(hits, root)
    calls = {os.path.basename(r[0]): list(r[2:]) for r in frame.itertuples(index=False)}
    assert calls['g1.fna'] == ['1', '1', '1', '1']                               # forward and reverse hits
    assert calls['g2.fna'] == ['2', '2', '1', '3']                               # lower-case contigs
    assert calls['g3.fna'] == ['-', '3', '3', '3']                               # nested allele suppressed; tuple in no profile
    assert calls['g4.fna'] == ['4', '4', '2', '2']                               # the short allele alone is reported
    assert calls['g5.fna'] == ['-', '1,2', '4,5', '1']                           # two copies; two numbers with one sequence
    assert calls['g6.fna'] == ['-', '-', '-', '4']                               # a mutant; an allele across a contig joint
    assert mlst.call_alleles(scheme, genomes).equals(frame)
    assert mlst.call_alleles(scheme, []).shape == (0, 6)


def test_host_scan_equals_a_find_loop():
    import pattern_scan_model as model
    rng = np.random.default_rng(3)
    text = model.random_text(rng, 3000, b'ACGT')
    patterns = [text[i:i + 20 + i % 9] for i in range(0, 2900, 131)] + [b'A' * 8, b'ACGTACGTAC', text[-9:], text[-9:] + b'A']
    for seed in (1, 4, 8):
        first, count = mlst.host_scan(text, patterns, seed)
        want = model.first_count(text, patterns)
        assert np.array_equal(first, want[0]) and np.array_equal(count, want[1])


def test_format_mlst_line():
    assert mlst.format_mlst_line('a/b.fna', 'demo', '-', ['x', 'y'], ['1,2', '-']) == 'a/b.fna\tdemo\t-\tx(1,2)\ty(-)'


def test_run_mlst_with_a_directory_and_with_a_list(golden_dir, tmp_path):
    root, scheme_dir, genomes = fixture(golden_dir)
    mlst.MLST_PATH_COUNTS.clear()
    frame = pa.run_mlst(genomes[::-1], str(tmp_path / 'list.tsv'), scheme_dir=scheme_dir)            # a list: in its order
    want = expected_lines(root).splitlines(True)
    assert open(tmp_path / 'list.tsv').read() == ''.join(want[::-1]) and frame['genome'].tolist() == genomes[::-1]
    frame = pa.run_mlst(os.path.join(root, 'genomes'), str(tmp_path / 'dir.tsv'), n_jobs=4, mlst_path='/nowhere/mlst',
                        env={'A': 'b'}, scheme_dir=scheme_dir, scheme='demo')                        # a directory: sorted
    assert open(tmp_path / 'dir.tsv').read() == ''.join(want) and frame['ST'].tolist() == ['1', '2', '-', '4', '-', '-']
    assert mlst.MLST_PATH_COUNTS == {'host': 12}
    with pytest.raises(ValueError, match='external'):
        pa.run_mlst(genomes, str(tmp_path / 'none.tsv'))
    assert not os.path.exists(tmp_path / 'none.tsv')


def test_load_scheme_errors(golden_dir, tmp_path):
    _, scheme_dir, _ = fixture(golden_dir)
    broken = tmp_path / 'no_tfa'
    shutil.copytree(scheme_dir, broken)
    os.remove(broken / 'defB.tfa')                                               # a locus between two loci without its file
    with pytest.raises(ValueError, match=r'demo\.txt:1: locus defB'):
        mlst.load_scheme(str(broken))
    broken = tmp_path / 'bad_number'
    shutil.copytree(scheme_dir, broken)
    with open(broken / 'ghiC.tfa', 'a') as f:
        f.write('>ghiC_x7\nACGTACGT\n')
    with pytest.raises(ValueError, match=r'ghiC\.tfa:13: '):
        mlst.load_scheme(str(broken))
    broken = tmp_path / 'other_locus'
    shutil.copytree(scheme_dir, broken)
    with open(broken / 'abcA.tfa', 'a') as f:
        f.write('>abcB_7\nACGTACGT\n')
    with pytest.raises(ValueError, match=r'abcA\.tfa:13: '):
        mlst.load_scheme(str(broken))
    broken = tmp_path / 'bad_profile'
    shutil.copytree(scheme_dir, broken)
    with open(broken / 'demo.txt', 'a') as f:
        f.write('6\t1\tnew\t1\t\t\n')
    with pytest.raises(ValueError, match=r'demo\.txt:7: '):
        mlst.load_scheme(str(broken))
    (tmp_path / 'two').mkdir()
    for name in ('a.txt', 'b.txt'):
        (tmp_path / 'two' / name).write_text('ST\tx\n')
    with pytest.raises(ValueError, match='name the scheme'):
        mlst.load_scheme(str(tmp_path / 'two'))


def test_an_allele_holding_the_joining_byte_is_refused(golden_dir):
    _, scheme_dir, genomes = fixture(golden_dir)
    scheme = mlst.load_scheme(scheme_dir)
    scheme.alleles['abcA'].append((9, b'ACGT\x00ACGT'))
    with pytest.raises(ValueError, match='0x00'):
        mlst.call_alleles(scheme, genomes[:1])


def test_an_allele_outside_the_complement_table_has_no_reverse_pattern(tmp_path):
    """`X` has no complement: the allele is found forward, and its would-be reverse complement is not searched"""
    allele = b'ACGTTGCAXACGGTCATTGACCAGTAGGATCCAAGTCTGA'
    scheme = mlst.Scheme('s', ['loc'], {'loc': [(1, allele)]}, {(1,): '7'})
    fake_rc = allele[::-1].translate(bytes.maketrans(b'ACGT', b'TGCA'))
    for name, seq in (('fwd', allele), ('rev', fake_rc)):
        (tmp_path / (name + '.fna')).write_bytes(b'>c1\nTTTTT' + seq + b'GGGG\n')
    frame = mlst.call_alleles(scheme, [str(tmp_path / 'fwd.fna'), str(tmp_path / 'rev.fna')])
    assert frame['ST'].tolist() == ['7', '-'] and frame['loc'].tolist() == ['1', '-']


def test_synthetic_scheme_round_trip(tmp_path):
    scheme = synth.mlst_scheme(n_loci=3, n_alleles=20, length=80, seed=5)
    synth.write_mlst_scheme(scheme, str(tmp_path / 'scheme'))
    assert mlst.load_scheme(str(tmp_path / 'scheme')) == scheme
    key, st = next(iter(scheme.profiles.items()))
    carried = {locus: (number, '+-'[i % 2]) for i, (locus, number) in enumerate(zip(scheme.loci, key))}
    paths = [synth.mlst_genome(scheme, str(tmp_path / 'a.fna'), carried, n_bp=5000, n_contigs=2),
             synth.mlst_genome(scheme, str(tmp_path / 'b.fna'), carried, n_bp=5000, n_contigs=2, novel=(scheme.loci[1],))]
    frame, hits = mlst.call_alleles(scheme, paths, return_hits=True)
    assert frame['ST'].tolist() == [st, '-'] and frame[scheme.loci[1]].tolist() == [str(key[1]), '-']
    assert hits['strand'].tolist() == ['+', '-', '+', '+', '+'] and (hits['copies'] == 1).all()
