"""pangenomix_amd.ncbi on the host: known answers of the model host_sw, the model against a score-only
Smith-Waterman and a full-matrix traceback with the same tie rules (tests/sw_reference.py), candidate_pairs against brute force, the
contract of bidirectional_blast, the recorded reports of tests/golden/blast and reciprocal_best_hits on them."""
import math
import os

import numpy as np
import pytest

from pangenomix_amd import ncbi, synth
from sw_reference import core, pack, random_pairs, score_only, self_score, sub, traceback_sw, two_letter_relatives


# ---- known answers ----------------------------------------------------------------------------------------------------------
def test_identical_sequences():
    s = core(50, 1)
    assert ncbi.host_sw(s, s).tolist() == [self_score(s), 0, 49, 0, 49, 50, 50, 0]
    assert ncbi.host_sw(s, s, stats=False).tolist() == [self_score(s), 0, 49, 0, 49, 0, 0, 0]


def test_one_substitution():
    q = core(25, 2) + b'W' + core(25, 3)
    s = q[:25] + b'A' + q[26:]
    want = self_score(q) - sub(b'W', b'W') + sub(b'W', b'A')
    assert sub(b'W', b'A') == -3
    assert ncbi.host_sw(q, s).tolist() == [want, 0, 50, 0, 50, 50, 51, 0]


@pytest.mark.parametrize('k', [1, 4, 9])
def test_one_planted_deletion(k):
    q = core(60, 4) + b'W' * k + core(60, 5)
    s = q[:60] + q[60 + k:]
    want = [self_score(s) - (11 + k), 0, 119 + k, 0, 119, 120, 120 + k, 1]
    assert ncbi.host_sw(q, s).tolist() == want
    # the same alignment with the sequences exchanged: an insertion
    assert ncbi.host_sw(s, q).tolist() == [want[0], 0, 119, 0, 119 + k, 120, 120 + k, 1]


def test_unrelated_flanks_on_both_sides():
    c = core(40, 6)
    q, s = b'W' * 7 + c + b'W' * 5, b'P' * 11 + c + b'P' * 3
    assert sub(b'W', b'P') < 0
    assert ncbi.host_sw(q, s).tolist() == [self_score(c), 7, 46, 11, 50, 40, 40, 0]


def test_no_positive_cell():
    assert ncbi.host_sw(b'WWWW', b'PPPPPP').tolist() == [0] * 8
    assert ncbi.host_sw(b'', b'PPPPPP').tolist() == [0] * 8
    forward, reverse = ncbi.search_reports(['q'], *pack([b'WWWWWWWW']), ['s'], *pack([b'WWWWWPPP']), evalue=1e-10)
    assert forward == [] and reverse == []


# ---- the model against two others (tests/sw_reference.py) -----------------------------------------------------------------------
def test_scores_against_a_score_only_smith_waterman():
    for q, s in random_pairs(60, b'ACGT', 40, 11) + random_pairs(30, b'ACDEFGHIKLMNPQRSTVWYBZX', 60, 12):
        got = ncbi.host_sw(q, s, stats=False)
        assert (int(got[0]), int(got[2]), int(got[4])) == score_only(q, s), (q, s)


def test_statistics_against_a_traceback_where_ties_are_everywhere():
    pairs = random_pairs(260, b'ACGT', 40, 13) + random_pairs(40, b'AC', 30, 14)
    gapped = 0
    for q, s in pairs:
        want = traceback_sw(q, s)
        assert ncbi.host_sw(q, s).tolist() == want, (q, s)
        gapped += want[7] > 0
    assert gapped > 30


def test_statistics_against_a_traceback_past_one_strip():
    """Two-letter relatives of 66..140 residues with one planted deletion of 1..5: longer than the kernel's strip, which
    the pairs above are not, and every one gapped."""
    pairs = two_letter_relatives()
    assert len(pairs) >= 8
    for q, s in pairs:
        assert 66 <= len(q) <= 140 and 1 <= len(q) - len(s) <= 5 and set(q) <= set(b'AC')
        want = traceback_sw(q, s)
        assert ncbi.host_sw(q, s).tolist() == want, (q, s)
        assert want[7] > 0, (q, s)


@pytest.mark.parametrize('word_size', [3, 5])
def test_candidate_pairs_against_brute_force(word_size):
    rng = np.random.default_rng(word_size)
    letters = np.frombuffer(b'ACDEFGHIKLBNZ', dtype=np.uint8)              # B is N's class and Z is E's: words over classes
    set1 = [letters[rng.integers(0, letters.size, int(n))].tobytes() for n in rng.integers(0, 30, 40)] + [b'AC', b'ACDEF']
    set2 = [letters[rng.integers(0, letters.size, int(n))].tobytes() for n in rng.integers(0, 30, 30)] + [b'AC', b'acdef']
    cls = ncbi.tables()[0]

    def words(s):
        c = cls[ncbi.letters_of(s)].tolist() if len(s) else []
        return {tuple(c[i:i + word_size]) for i in range(len(c) - word_size + 1)}
    w1, w2 = [words(s) for s in set1], [words(s) for s in set2]
    want = sorted((a, b) for a in range(len(set1)) for b in range(len(set2)) if w1[a] & w2[b])
    pa, pb = ncbi.candidate_pairs(*pack(set1), *pack(set2), word_size=word_size)
    assert list(zip(pa.tolist(), pb.tolist())) == want
    assert want and len(want) < len(set1) * len(set2)
    assert not any(len(set1[a]) < word_size or len(set2[b]) < word_size for a, b in want)
    assert (len(set1) - 1, len(set2) - 1) in want or word_size > 5            # ACDEF / acdef: case does not matter


def test_candidate_pairs_refuses_other_word_sizes():
    for word_size in (2, 7):
        with pytest.raises(ValueError, match='word_size'):
            ncbi.candidate_pairs(*pack([b'ACDEFGH']), *pack([b'ACDEFGH']), word_size=word_size)


# ---- the function's contract ----------------------------------------------------------------------------------------------------
def write_faa(path, records):
    with open(path, 'w') as f:
        for header, s in records:
            f.write('>%s\n%s\n' % (header, s.decode('ascii')))
    return str(path)


def test_paths_directories_and_return_value(tmp_path, capsys):
    (tmp_path / 'in').mkdir()
    p = core(80, 20)
    one = write_faa(tmp_path / 'in' / 'strain.one.faa', [('x1 first protein', p), ('x2', core(70, 21))])
    two = write_faa(tmp_path / 'in' / 'two.faa', [('y1\tother', core(70, 22)), ('y2 copy', p)])
    report_dir = str(tmp_path / 'reports')
    got = ncbi.bidirectional_blast(one, two, report_dir, seq1_blast_db=str(tmp_path / 'db1'), seq2_blast_db=str(tmp_path / 'db2') + '/')
    assert got == (report_dir + '/strain.one_to_two.tsv', report_dir + '/two_to_strain.one.tsv')
    assert os.path.isdir(report_dir) and os.listdir(str(tmp_path / 'db1')) == [] and os.listdir(str(tmp_path / 'db2')) == []
    assert sorted(os.listdir(str(tmp_path / 'in'))) == ['strain.one.faa', 'two.faa']           # no database files
    printed = capsys.readouterr().out.splitlines()
    assert printed == [
        str(['blastp', '-db', str(tmp_path / 'db2') + '/two.faa', '-query', one, '-out', got[0], '-outfmt', '6',
             '-evalue', '1e-10', '-num_threads', '1']),
        str(['blastp', '-db', str(tmp_path / 'db1') + '/strain.one.faa', '-query', two, '-out', got[1], '-outfmt', '6',
             '-evalue', '1e-10', '-num_threads', '1'])]
    fields = open(got[0]).read().rstrip('\n').split('\t')
    assert fields[:10] == ['x1', 'y2', '100.000', '80', '0', '0', '1', '80', '1', '80']          # ids: the first token
    score = self_score(p)
    e = ncbi.K * 80 * 150 * math.exp(-ncbi.LAMBDA * score)
    assert fields[10:] == ['%.3g' % e, '%.1f' % ((ncbi.LAMBDA * score - math.log(ncbi.K)) / math.log(2))]
    assert open(got[1]).read().split('\t')[:2] == ['y2', 'x1']
    # without database directories the FASTA files' own directory is used, and it exists
    assert ncbi.bidirectional_blast(one, two, report_dir + '/') == got


def test_rejected_keys_and_nucleotides(tmp_path):
    one = write_faa(tmp_path / 'one.faa', [('x', core(50, 23))])
    for params in ({'outfmt': 7}, {'evalue': 1e-5, 'seg': 'yes'}, {'matrix': 'BLOSUM45'}, {'gapopen': 10}, {'gapextend': 2},
                   {'word_size': 2}, {'max_target_seqs': 0}):
        with pytest.raises(ValueError):
            ncbi.bidirectional_blast(one, one, str(tmp_path / 'r'), blast_params=params)
    accepted = {'matrix': 'BLOSUM62', 'gapopen': 11, 'gapextend': 1, 'num_threads': 8, 'word_size': 3}
    ncbi.bidirectional_blast(one, one, str(tmp_path / 'r'), blast_params=accepted)
    fna = write_faa(tmp_path / 'one.fna', [('x', b'ACGTACGTACGT')])
    with pytest.raises(ValueError, match='only protein'):
        ncbi.bidirectional_blast(fna, fna, str(tmp_path / 'r'))


def test_max_target_seqs_and_the_order_of_a_querys_lines(tmp_path):
    p = core(90, 24)
    worse = p[:30] + b'W' + p[31:60] + b'W' + p[61:]
    one = write_faa(tmp_path / 'one.faa', [('q', p)])
    two = write_faa(tmp_path / 'two.faa', [('worse', worse), ('same1', p), ('other', core(90, 25)), ('same2', p)])
    forward, _ = ncbi.bidirectional_blast(one, two, str(tmp_path / 'r'))
    assert [line.split('\t')[1] for line in open(forward)] == ['same1', 'same2', 'worse']      # E, then score, then file order
    forward, reverse = ncbi.bidirectional_blast(one, two, str(tmp_path / 'r'), blast_params={'max_target_seqs': 2})
    assert [line.split('\t')[1] for line in open(forward)] == ['same1', 'same2']
    assert [line.split('\t')[0] for line in open(reverse)] == ['worse', 'same1', 'same2']       # queries in file order


def test_an_evalue_that_cuts_one_direction_only(tmp_path):
    """E = K * len(query) * residues of the other set * exp(-lambda S): a short protein of a small set against a long one
    of a large set has a far larger E forward than in reverse."""
    p = core(30, 26)
    long_one = core(500, 27) + p + core(500, 28)
    filler = [('f%d' % i, core(400, 30 + i)) for i in range(20)]
    one = write_faa(tmp_path / 'one.faa', [('short', p)])
    two = write_faa(tmp_path / 'two.faa', [('long', long_one)] + filler)
    score = int(ncbi.host_sw(p, long_one)[0])
    forward_e = ncbi.K * 30 * (1030 + 8000) * math.exp(-ncbi.LAMBDA * score)
    reverse_e = ncbi.K * 1030 * 30 * math.exp(-ncbi.LAMBDA * score)
    assert forward_e > 5 * reverse_e
    between = math.sqrt(forward_e * reverse_e)
    forward, reverse = ncbi.bidirectional_blast(one, two, str(tmp_path / 'r'), blast_params={'evalue': between})
    assert open(forward).read() == ''
    assert [line.split('\t')[:2] for line in open(reverse)] == [['long', 'short']]
    forward, reverse = ncbi.bidirectional_blast(one, two, str(tmp_path / 'r'), blast_params={'evalue': forward_e * 1.01})
    assert [line.split('\t')[:2] for line in open(forward)] == [['short', 'long']]


# ---- the recorded fixture -------------------------------------------------------------------------------------------------------
def test_the_recorded_reports(golden_dir, tmp_path):
    src = os.path.join(golden_dir, 'blast')
    forward, reverse = ncbi.bidirectional_blast(os.path.join(src, 'a.faa'), os.path.join(src, 'b.faa'), str(tmp_path / 'out'))
    assert open(forward).read() == open(os.path.join(src, 'a_to_b.tsv')).read()
    assert open(reverse).read() == open(os.path.join(src, 'b_to_a.tsv')).read()
    lines = {line.split('\t')[0]: line.rstrip('\n').split('\t') for line in open(forward)}
    # by hand: a10 is in b unchanged (120 residues), a11 without its residues 41..45 (one gap of five, no mismatch)
    assert lines['a10'][1:10] == ['b_same', '100.000', '120', '0', '0', '1', '120', '1', '120']
    assert lines['a11'][1:10] == ['b_del5', '%.3f' % (100 * 148 / 153.0), '153', '0', '1', '1', '153', '1', '148']
    assert 'a8' not in lines and 'a9' not in lines                          # left out of b


def test_reciprocal_best_hits_on_the_recorded_reports(golden_dir):
    src = os.path.join(golden_dir, 'blast')
    got = ncbi.reciprocal_best_hits(os.path.join(src, 'a_to_b.tsv'), os.path.join(src, 'b_to_a.tsv'))
    origin = dict(line.split() for line in open(os.path.join(src, 'origin.tsv')))
    assert list(got.columns) == ['seq1', 'seq2', 'pident', 'length', 'evalue', 'bitscore']
    assert {b: a for a, b in zip(got['seq1'], got['seq2'])} == origin
    assert got['seq1'].tolist() == [line.split('\t')[0] for line in open(os.path.join(src, 'a_to_b.tsv'))]


def test_reciprocal_best_hits_needs_both_directions(tmp_path):
    row = '%s\t%s\t100.000\t50\t0\t0\t1\t50\t1\t50\t1e-30\t100.0\n'
    forward, reverse = tmp_path / 'f.tsv', tmp_path / 'r.tsv'
    forward.write_text(row % ('a1', 'b1') + row % ('a1', 'b2') + row % ('a2', 'b1') + row % ('a3', 'b3'))
    reverse.write_text(row % ('b1', 'a1') + row % ('b2', 'a1') + row % ('b3', 'a4'))
    got = ncbi.reciprocal_best_hits(str(forward), str(reverse))
    assert list(zip(got['seq1'], got['seq2'])) == [('a1', 'b1')]


def test_related_protein_set_is_deterministic_and_related():
    base = synth.protein_set('tiny').genome(0)[1][:30]
    names, seqs, origin = synth.related_protein_set(base, seed=5)
    again = synth.related_protein_set(base, seed=5)
    assert (names, seqs, origin.tolist()) == (again[0], again[1], again[2].tolist())
    assert 0 < len(seqs) < len(base) and sorted(set(origin.tolist())) == sorted(origin.tolist())
    long_ones = [(s, base[k]) for s, k in zip(seqs, origin) if len(base[k]) >= 60][:5]
    for s, b in long_ones:
        r = ncbi.host_sw(b, s)
        assert r[5] > 0.7 * len(b) and r[6] >= r[5]
