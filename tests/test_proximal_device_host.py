"""The ctx= layer of the 5'/3' UTR pangenome builders (pangenomix_amd.pangenome) without a device: a stand-in
context runs the plain-Python models of the two library calls (tests/prox_model.py), so what is checked here is everything
between the files and those calls -- the vectorised parsers, the window arithmetic, the regular-input rule and its
fall-backs, the files put together as bytes. Against what the reference wrote, printed and raised (tests/golden/proximal,
tests/golden/proximal_device) and against the host path (ctx=None)."""
import json
import os
import shutil

import numpy as np
import pytest

import prox_model as model
from pangenomix_amd import pangenome as pg
from test_host_golden import assert_same_npz, same_file
from test_proximal_golden import GENOMES, RUNS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
RECORDED = model.recorded_runs(GOLDEN)


@pytest.mark.parametrize('tag', sorted(RECORDED))
def test_recorded_runs_through_the_stub(tag, tmp_path, golden_dir, capsys):
    ctx = model.StubContext()
    model.run_recorded(RECORDED[tag], ctx, tmp_path, golden_dir, capsys)
    assert ctx.calls['prox_cut'] > 0 or RECORDED[tag]['genomes'][0] in RECORDED[tag]['host']


def test_every_case_the_fixtures_are_there_for_is_in_them():
    assert {len(r['host']) for r in RECORDED.values()} == {0, 1, 2}
    assert sum(1 for r in RECORDED.values() if r['raised']) == 2
    assert {r['kw'].get('max_overlap', -1) for r in RECORDED.values()} == {-1, 0, 5}
    assert {r['side'] for r in RECORDED.values()} == {'upstream', 'downstream'}
    assert {bool(r['kw'].get('include_fragments')) for r in RECORDED.values()} == {False, True}


@pytest.mark.parametrize('tag', sorted(RUNS))
def test_first_fixtures_through_the_stub(tag, tmp_path, golden_dir, capsys):
    """tests/test_proximal_golden.py with ctx=: the same files, labels, members and stdout, all on the device path"""
    fn, kw, name, side, footer = RUNS[tag]
    din = tmp_path / 'in'
    shutil.copytree(os.path.join(golden_dir, 'proximal', 'in'), din)
    exp = os.path.join(golden_dir, 'proximal', 'expected', tag)
    out = tmp_path / 'out'
    out.mkdir()
    pairs = [(str(din / (g + '.gff')), str(din / (g + '.fna'))) for g in GENOMES]
    capsys.readouterr()
    pg.PROXIMAL_PATH_COUNTS.clear()
    df = fn(pairs, str(din / 'T_allele_names.tsv'), str(out), ctx=model.StubContext(), **kw)
    printed = capsys.readouterr().out.replace(str(din), '<in>').replace(str(out), '<out>')
    assert printed == json.load(open(os.path.join(golden_dir, 'proximal', 'expected', 'stdout.json')))[tag]
    assert dict(pg.PROXIMAL_PATH_COUNTS) == {'extract_device': 3, 'consolidate_device': 1}
    for g in GENOMES:
        f = '%s_%s%s.fna' % (g, side, footer)
        same_file(str(din / 'derived' / f), os.path.join(exp, f))
    same_file(str(out / ('%s_nr_%s.fna' % (name, side))), os.path.join(exp, '%s_nr_%s.fna' % (name, side)))
    npz = '%s_strain_by_%s.npz' % (name, side)
    same_file(str(out / (npz + '.labels.txt')), os.path.join(exp, npz + '.labels.txt'))
    assert_same_npz(str(out / npz), os.path.join(exp, npz))
    assert list(df.columns) == ['p10', 'p1', 'p2']


def test_generated_genomes_against_the_host_path(tmp_path, capsys):
    model.compare_with_host_path(model.StubContext(), tmp_path, capsys)


def test_beyond_the_limits_of_the_library_the_host_path_runs(tmp_path, golden_dir, capsys):
    """a context that refuses more than 3 windows / records, as the library refuses 2^24: same files, all by the host"""
    ctx = model.StubContext(max_n=3)
    model.run_recorded(RECORDED['upstream_mo5'], ctx, tmp_path, golden_dir, capsys, all_by_the_host=True)
    assert ctx.calls == {'prox_cut': 5, 'prox_group': 2}     # (asked, and refused)
    # the module's own limits, checked before the library is asked, are the library's
    assert (pg._PROX_MAX_RECORDS, pg._PROX_MAX_BYTES, pg._PROX_MAX_GENES) == (1 << 24, 1 << 32, 1 << 24)


def test_the_module_s_own_limits_are_checked_before_the_library_is_asked(tmp_path, golden_dir, capsys, monkeypatch):
    monkeypatch.setattr(pg, '_PROX_MAX_RECORDS', 3)
    ctx = model.StubContext()
    model.run_recorded(RECORDED['downstream_mo0'], ctx, tmp_path, golden_dir, capsys, all_by_the_host=True)
    assert ctx.calls == {'prox_cut': 0, 'prox_group': 0}


# -- one genome: what makes it irregular, and that the host's answer is then the answer -------------------------------------------
def _edit(text, old, new):
    assert text.count(old) >= 1, old
    return text.replace(old, new, 1)


GFF_EDITS = {
    'eight fields': lambda t: _edit(t, '\t0\tID=fig|q1.peg.3', '\tID=fig|q1.peg.3'),
    'ten fields': lambda t: _edit(t, 'ID=fig|q1.peg.3;', 'x\tID=fig|q1.peg.3;'),
    'coordinate with a sign': lambda t: _edit(t, '\t84\t', '\t+84\t'),
    'coordinate with a blank': lambda t: _edit(t, '\t84\t', '\t 84\t'),
    'coordinate not a number': lambda t: _edit(t, '\t110\t', '\t11o\t'),
    'strand .': lambda t: _edit(t, '84\t110\t.\t+', '84\t110\t.\t.'),
    'attribute without =': lambda t: _edit(t, 'ID=fig|q1.peg.3;product=x y', 'ID=fig|q1.peg.3;product'),
    'attribute with two =': lambda t: _edit(t, 'ID=fig|q1.peg.3;product=x y', 'ID=fig|q1.peg.3;product=x=y'),
    'no ID': lambda t: _edit(t, 'ID=fig|q1.peg.3;', 'Id=fig|q1.peg.3;'),
    'two CDS with one start and stop': lambda t: t + t.split('\n')[4] + '\n',
    'indented line': lambda t: _edit(t, 'accn|c1\tPATRIC\tCDS\t84', ' accn|c1\tPATRIC\tCDS\t84'),
    'carriage returns': lambda t: t.replace('\n', '\r\n'),
    'not ASCII': lambda t: _edit(t, 'product=x y', 'product=x é'),
}
GFF_REGULAR_EDITS = {
    'nothing': lambda t: t,
    'ID given twice: the later one counts': lambda t: _edit(t, 'ID=fig|q1.peg.3;', 'ID=fig|q1.peg.2;ID=fig|q1.peg.3;'),
    'ID last': lambda t: _edit(t, 'ID=fig|q1.peg.3;product=x y', 'product=x y;ID=fig|q1.peg.3'),
    'no pipe in the contig': lambda t: t.replace('accn|', ''),
    'two pipes in the contig': lambda t: t.replace('accn|', 'a|b|'),
    'leading zeros': lambda t: _edit(t, '\t84\t', '\t0084\t'),
    'no newline at the end': lambda t: t.rstrip('\n'),
    'comment with tabs, blank lines': lambda t: _edit(t, '\n\n', '\n\n#a\tb\n\n\n'),
}


def _extract_both_ways(tmp_path, golden_dir, capsys, gff_text, fna_bytes, feat, **kw):
    (tmp_path / 'g.gff').write_bytes(gff_text.encode('utf-8'))
    (tmp_path / 'g.fna').write_bytes(fna_bytes)
    results = []
    for which in (None, model.StubContext()):
        out = tmp_path / ('out_%s.fna' % ('host' if which is None else 'ctx'))
        capsys.readouterr()
        pg.PROXIMAL_PATH_COUNTS.clear()
        raised = None
        try:
            pg.extract_upstream_sequences(str(tmp_path / 'g.gff'), str(tmp_path / 'g.fna'), str(out), limits=(-20, 3),
                                          feature_to_allele=feat, ctx=which, **kw)
        except Exception as e:                               # noqa: BLE001 -- the two paths must raise the same
            raised = (type(e), [str(a) for a in e.args])
        results.append((raised, out.read_bytes() if out.exists() else None, capsys.readouterr().out))
    assert results[0] == results[1]
    return dict(pg.PROXIMAL_PATH_COUNTS), results[1]


@pytest.mark.parametrize('max_overlap', (-1, 5))
@pytest.mark.parametrize('what', sorted(GFF_EDITS))
def test_irregular_gff_goes_to_the_host(what, max_overlap, tmp_path, golden_dir, capsys):
    din = os.path.join(golden_dir, 'proximal_device', 'in')
    feat = pg.__load_feature_to_allele__(os.path.join(din, 'T_allele_names.tsv'))
    text = GFF_EDITS[what](open(os.path.join(din, 'q1.gff')).read())
    counts, _ = _extract_both_ways(tmp_path, golden_dir, capsys, text, open(os.path.join(din, 'q1.fna'), 'rb').read(), feat,
                                   max_overlap=max_overlap)
    regular_without_overlap = what == 'two CDS with one start and stop' and max_overlap < 0
    assert counts == ({'extract_device': 1} if regular_without_overlap else {'extract_host': 1})


@pytest.mark.parametrize('what', sorted(GFF_REGULAR_EDITS))
def test_regular_gff_stays_on_the_device(what, tmp_path, golden_dir, capsys):
    din = os.path.join(golden_dir, 'proximal_device', 'in')
    feat = pg.__load_feature_to_allele__(os.path.join(din, 'T_allele_names.tsv'))
    text = GFF_REGULAR_EDITS[what](open(os.path.join(din, 'q1.gff')).read())
    counts, (raised, written, printed) = _extract_both_ways(tmp_path, golden_dir, capsys, text,
                                                            open(os.path.join(din, 'q1.fna'), 'rb').read(), feat, max_overlap=5)
    assert counts == {'extract_device': 1} and raised is None and printed.startswith('Loaded upstream sequences: ')
    assert written.count(b'>') == 8                          # (the contig is what follows the last '|', if there is one)


@pytest.mark.parametrize('what,edit,regular', [
    ('a contig given twice: the later one counts', lambda b: b + b'>c1\n' + b'ACGTTGCA' * 30 + b'\n', True),
    ('a header and no sequence', lambda b: b + b'>c7\n>c8 x\n', True),
    ('no newline at the end', lambda b: b.rstrip(b'\n'), True),
    ('an empty file', lambda b: b'', True),
    ('lines before the first header', lambda b: b'ACGT\n' + b, False),
    ('a header without a name', lambda b: b + b'> \nACGT\n', False),
    ('a blank at the end of a line', lambda b: b.replace(b'\n', b' \n', 2), False),
    ('a tab inside a line', lambda b: b[:40] + b'\t' + b[40:], False),
    ('a separator only str.strip() strips', lambda b: b[:40] + b'\x1c' + b[40:], False),
    ('not ASCII', lambda b: b[:40] + b'\xc3\xa9' + b[40:], False),
])
def test_fna_regular_or_not(what, edit, regular, tmp_path, golden_dir, capsys):
    din = os.path.join(golden_dir, 'proximal_device', 'in')
    feat = pg.__load_feature_to_allele__(os.path.join(din, 'T_allele_names.tsv'))
    counts, _ = _extract_both_ways(tmp_path, golden_dir, capsys, open(os.path.join(din, 'q1.gff')).read(),
                                   edit(open(os.path.join(din, 'q1.fna'), 'rb').read()), feat, max_overlap=0)
    assert counts == ({'extract_device': 1} if regular else {'extract_host': 1})


def test_without_a_mapping_the_host_raises_its_type_error(tmp_path, golden_dir, capsys):
    din = os.path.join(golden_dir, 'proximal_device', 'in')
    counts, (raised, _, _) = _extract_both_ways(tmp_path, golden_dir, capsys, open(os.path.join(din, 'q1.gff')).read(),
                                                open(os.path.join(din, 'q1.fna'), 'rb').read(), None)
    assert raised[0] is TypeError and counts == {'extract_host': 1}


def test_allele_names_file_instead_of_a_mapping(tmp_path, golden_dir, capsys):
    din = os.path.join(golden_dir, 'proximal_device', 'in')
    out = tmp_path / 'd.fna'
    pg.PROXIMAL_PATH_COUNTS.clear()
    pg.extract_downstream_sequences(os.path.join(din, 'q3.gff'), os.path.join(din, 'q3.fna'), str(out), limits=(-3, 20),
                                    max_overlap=5, allele_names=os.path.join(din, 'T_allele_names.tsv'), ctx=model.StubContext())
    same_file(str(out), os.path.join(golden_dir, 'proximal_device', 'expected', 'downstream_mo5', 'q3_downstream.fna'))
    assert dict(pg.PROXIMAL_PATH_COUNTS) == {'extract_device': 1}


# -- consolidation ------------------------------------------------------------------------------------------------------------
def _consolidate_both_ways(tmp_path, capsys, files, feat, side='upstream'):
    results = []
    for which in (None, model.StubContext()):
        d = tmp_path / ('host' if which is None else 'ctx')
        d.mkdir()
        paths = []
        for name, data in files.items():
            (d / name).write_bytes(data)
            paths.append(str(d / name))
        capsys.readouterr()
        pg.PROXIMAL_PATH_COUNTS.clear()
        raised, table = None, None
        try:
            df = pg.consolidate_proximal(paths, str(d / 'nr.fna'), feat, side, ctx=which)
            table = (list(df.index), list(df.columns), df.data.row.tolist(), df.data.col.tolist(), df.data.data.tolist(),
                     df.data.shape)
        except Exception as e:                               # noqa: BLE001 -- the two paths must raise the same
            raised = (type(e), [str(a) for a in e.args])
        results.append((raised, table, (d / 'nr.fna').read_bytes() if (d / 'nr.fna').exists() else None, capsys.readouterr().out))
    assert results[0] == results[1]
    return dict(pg.PROXIMAL_PATH_COUNTS), results[1]


FOOT = b'_upstream(-20,3)\n'
FEAT = {'f|a.1': 'T_C1A0', 'f|a.2': 'T_C10A0', 'f|b.1': 'T_C1A1', 'f|b.2': 'T_C2A0', 'f|b.3': 'X_C2A0', 'f|b.4': 'plainA7', '': 'T_C5A0'}
FILE_A = b'>f|a.1' + FOOT + b'ACGT\nAC\n>f|a.2' + FOOT + b'\n>f|a.1' + FOOT + b'ACGTAC\n>f|a.2' + FOOT
FILE_B = b'>f|b.1' + FOOT + b'ACGTAC\n>f|b.2' + FOOT + b'ACGTAC\n>f|b.1' + FOOT + b'TT\n'


@pytest.mark.parametrize('what,files,regular', [
    ('two files', {'a_upstream.fna': FILE_A, 'b_upstream.fna': FILE_B}, True),
    ('no newline at the end', {'a_upstream.fna': FILE_A[:-1], 'b_upstream.fna': FILE_B[:-1]}, True),
    ('two prefixes: names sorted by Python', {'a_upstream.fna': FILE_A, 'b_upstream.fna': FILE_B + b'>f|b.3' + FOOT + b'GG\n'}, True),
    ('a gene that is not <prefix>C<int>', {'b_upstream.fna': FILE_B + b'>f|b.4' + FOOT + b'GG\n'}, True),
    ('lines before the first header, the feature of which is mapped', {'a_upstream.fna': b'GGG\n' + FILE_A}, True),
    ('an empty file', {'a_upstream.fna': FILE_A, 'b_upstream.fna': b''}, False),
    ('a feature without an allele', {'a_upstream.fna': FILE_A + b'>f|zz' + FOOT + b'AC\n'}, False),
    ('two files, one genome name', {'a_upstream.fna': FILE_A, 'a_upstream_2.fna': FILE_B}, False),
    ('carriage returns', {'a_upstream.fna': FILE_A.replace(b'\n', b'\r\n')}, False),
    ('a blank at the end of a sequence line', {'a_upstream.fna': FILE_A.replace(b'ACGT\n', b'ACGT \n')}, False),
    ('not ASCII', {'a_upstream.fna': FILE_A + b'>f|\xc3\xa9' + FOOT + b'AC\n'}, False),
])
def test_consolidation_regular_or_not(what, files, regular, tmp_path, capsys):
    counts, (raised, table, nr, printed) = _consolidate_both_ways(tmp_path, capsys, files, FEAT)
    assert counts == ({'consolidate_device': 1} if regular else {'consolidate_host': 1})
    if regular:
        assert raised is None and printed == 'Sparsifying upstream table...\nBuilding binary matrix...\n'
    if what == 'two files':
        assert table[0] == ['T_C10U0', 'T_C1U0', 'T_C1U1', 'T_C2U0'] and table[1] == ['a', 'b']
        assert nr == b'>T_C1U0\nACGTAC\n>T_C10U0\n\n>T_C2U0\nACGTAC\n>T_C1U1\nTT\n'


def test_sparr_is_still_refused_where_the_host_refuses_it(tmp_path, capsys):
    for which in (None, model.StubContext()):
        d = tmp_path / str(which is None)
        d.mkdir()
        (d / 'a_upstream.fna').write_bytes(FILE_A)
        with pytest.raises(NotImplementedError):
            pg.consolidate_proximal([str(d / 'a_upstream.fna')], str(d / 'nr.fna'), FEAT, 'upstream', output_format='sparr', ctx=which)
        assert (d / 'nr.fna').exists()


def test_models_agree_with_the_module_s_own_helpers():
    rng = np.random.default_rng(9)
    letters = np.frombuffer(model.LETTERS, dtype=np.uint8)
    seq = letters[rng.integers(0, 22, 200)].tobytes()
    out, off, bad = model.cut(seq, [3, 50], [40, 60], [1, 1])
    assert out[:40].decode() == pg.reverse_complement(seq[3:43].decode()) and not bad.any()
    first, variant, distinct = model.group([b'A', b'C', b'A', b'A', b'G'], [1, 1, 2, 1, 1])
    assert first.tolist() == [0, 1, 2, 0, 4] and variant.tolist() == [0, 1, 0, 0, 2] and distinct == 4
