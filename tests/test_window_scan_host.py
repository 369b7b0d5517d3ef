"""The host side of the direct UTR table validators (pangenomix_amd.pangenome.validate_proximal_table_direct)
without a device: the Python restatement of the reference's loop (tests/window_scan_model.py) against what the reference
itself printed and raised (tests/golden/proximal_direct), and the validators' own host work -- key construction, the rule for
sequences shorter than the window, the order of the errors -- with the model's scan standing in for the device."""
import numpy as np
import pytest

import window_scan_model as model
from pangenomix_amd import pangenome as pg

CASES = model.load_cases()


@pytest.mark.parametrize('name', sorted(CASES))
def test_model_prints_and_raises_what_the_reference_did(name):
    case = CASES[name]
    genomes, nr = model.case_paths(case)
    out, exc = [], None
    try:
        model.validate_direct(case['index'], case['columns'], [tuple(c) for c in case['cells']], genomes, nr, case['limits'],
                              case['side'], case['log_group'], out=out)
    except KeyError as e:
        exc = e
    assert ''.join(out).replace(model.GOLDEN, '<golden>') == case['stdout']
    if case['exception'] is None:
        assert exc is None
    else:
        assert type(exc).__name__ == case['exception']['type'] and exc.args[0] == case['exception']['arg']


def test_the_golden_cases_cover_what_they_should():
    assert len(CASES) >= 20
    assert sorted(c['exception']['arg'] for c in CASES.values() if c['exception']) == ['T_C90D0', 'X', 'p7']
    shared = CASES['up_two_genes_share_a_sequence']['stdout']
    assert '\tMissing T_C99U0 from p1\n\tMissing T_C97U0 from p1\n' in shared and 'T_C98U0 from p1' not in shared
    assert 'Computing' not in CASES['up_no_tally_limits_51_2']['stdout']


@pytest.mark.parametrize('table', ('frame', 'lsdf'))
@pytest.mark.parametrize('name', sorted(CASES))
def test_validator_with_the_model_scan_equals_the_reference(name, table, capsys):
    case = CASES[name]
    ctx = model.ModelContext()
    df = model.case_frame(case) if table == 'frame' else model.case_lsdf(case)
    printed, result, exc = model.run_validator(pg.validate_proximal_table_direct, case, df, capsys, limits=tuple(case['limits']),
                                               side=case['side'], log_group=case['log_group'], ctx=ctx)
    model.assert_as_recorded(case, printed, result, exc)
    for text, keys in ctx.calls:                    # one call per genome at the most, never a key with the joining byte
        assert keys.shape[1] == case['limits'][1] - case['limits'][0] and not (keys == 0).any()
    assert len(ctx.calls) <= len(case['genomes'])


def test_scan_keys_reverse_shared_and_unknown():
    w = 6
    seqs = ['AACCGG', 'CCGGTT', 'ACGCGT', 'AAXCGG', 'acgtwn', 'AACéGG']
    #        P         rc(P): shares both rows   palindrome: one row   X: no reverse   lower case + ambiguity   not ASCII: none
    keys, fwd, rev = pg._scan_keys(seqs, w)
    rows = [bytes(k) for k in keys]
    assert len(set(rows)) == len(rows) and keys.dtype == np.uint8 and keys.shape[1] == w
    assert rows[fwd[0]] == b'AACCGG' and rows[rev[0]] == b'CCGGTT'
    assert fwd[1] == rev[0] and rev[1] == fwd[0]
    assert fwd[2] == rev[2] and rows[fwd[2]] == b'ACGCGT'
    assert rows[fwd[3]] == b'AAXCGG' and rev[3] == -1
    assert rows[fwd[4]] == b'acgtwn' and rows[rev[4]] == b'nwacgt'
    assert fwd[5] == -1 and rev[5] == -1
    assert len(rows) == 2 + 1 + 1 + 2
    with pytest.raises(ValueError, match='0x00'):
        pg._scan_keys(['AC\x00TAG'], w)
    keys, fwd, rev = pg._scan_keys([], w)
    assert keys.shape == (0, w)


def test_genome_scan_joins_contigs_with_a_byte_no_key_holds():
    ctx = model.ModelContext()
    contigs = ['AAAACCCC', 'GGGGTTTA']
    seqs = ['AACC', 'CCGG', 'TAAA', 'GGTT', 'CCCC', 'ACGT']
    #        in c1   across the joint: no   rc(TTTA): yes   both strands   rc(GGGG)   absent
    found = pg._genome_missing(seqs, contigs, 4, lambda text, keys: ctx.window_scan(text, keys))
    assert found == [True, False, True, True, True, False]
    assert ctx.calls[0][0] == b'AAAACCCC\x00GGGGTTTA' and len(ctx.calls) == 1
    assert pg._genome_missing(seqs, [], 4, None) == [False] * 6          # no contigs, no call
    assert pg._genome_missing([], contigs, 4, None) == []


def test_short_sequence_rule():
    contigs = ['ACGTTGCAAG', 'GGA']
    window = 8
    scan = lambda text, keys: model.scan(text, keys, window)            # noqa: E731
    cases = {'CAAG': True,        # suffix of a contig
             'ACGTT': False,      # a prefix is not
             'GTTG': False,       # nor the middle
             'ACGTTGCAAG': False,  # longer than the window: never
             'CGT': True,         # rc('ACG') = 'CGT': the reverse complement of a contig's prefix
             'TCC': True,         # rc('GGA'): the whole short contig, reversed
             'GGA': True,         # the whole short contig
             'CTTG': False,       # rc of a SUFFIX: a prefix of the reverse complement
             'GGAT': False}       # longer than the contig it begins
    seqs = list(cases)
    assert pg._genome_missing(seqs, contigs, window, scan) == [cases[s] for s in seqs]
    # and the str-slicing restatement of the reference agrees
    for s, want in cases.items():
        slices = set()
        for c in contigs:
            for strand in (c, model.reverse_complement(c)):
                slices.update(strand[i:i + window] for i in range(len(strand)))
        assert (s in slices) == want, s


def test_key_errors_come_in_the_reference_order(tmp_path, capsys):
    """per genome: Evaluating line, then KeyError(genome), then KeyError(label), then KeyError(base) of the first offending
    character of the first offending contig -- before any of that genome's Missing lines, after the earlier genomes' output"""
    import pandas as pd
    (tmp_path / 'a.fna').write_text('>c1\nACGTACGTAC\n')
    (tmp_path / 'b.fna').write_text('>c1\nACGTAC\n>c2\nACQTAZGT\n>c3\nXA\n')
    (tmp_path / 'nr.fna').write_text('>r1\nACGT\n>r2\nTTTT\n')
    paths = [str(tmp_path / 'a.fna'), str(tmp_path / 'b.fna')]
    nr = str(tmp_path / 'nr.fna')
    ctx = model.ModelContext()

    def run(df):
        capsys.readouterr()
        with pytest.raises(KeyError) as e:
            pg.validate_proximal_table_direct(df, paths, nr, (-2, 2), 'upstream', ctx=ctx)
        return e.value.args[0], capsys.readouterr().out
    head = 'Loading upstream sequences...\n1 Evaluating a %s\n\tMissing r2 from a\n2 Evaluating b %s\n' % tuple(paths)
    nan = float('nan')
    assert run(pd.DataFrame([[1, 1], [1, 1]], index=['r1', 'r2'], columns=['a', 'b'])) == ('Q', head)
    assert run(pd.DataFrame([[1, 1], [1, 1], [nan, 1]], index=['r1', 'r2', 'r9'], columns=['a', 'b'])) == ('r9', head)
    assert run(pd.DataFrame([[1], [1], [nan]], index=['r1', 'r2', 'r9'], columns=['a'])) == ('b', head)
    # a genome with nothing recorded still has its contigs checked (the reference complements every contig)
    assert run(pd.DataFrame([[1, nan], [1, nan]], index=['r1', 'r2'], columns=['a', 'b'])) == ('Q', head)


def test_wrappers_call_the_direct_function(capsys):
    """the reference's wrappers raise NameError (they call validate_proximal_table); here they are the direct call with
    their side and default limits"""
    for name, fn, side in (('up_consistent_lg1', pg.validate_upstream_table_direct, 'upstream'),
                           ('down_consistent_lg2', pg.validate_downstream_table_direct, 'downstream')):
        case = CASES[name]
        printed, result, exc = model.run_validator(fn, case, model.case_frame(case), capsys, log_group=case['log_group'],
                                                   ctx=model.ModelContext())
        model.assert_as_recorded(case, printed, result, exc)
    with pytest.raises(ValueError, match='limits'):
        pg.validate_upstream_table_direct(model.case_frame(case), [], model.case_paths(case)[1], limits=(0, 1025))
