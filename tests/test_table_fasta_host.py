"""The host side of the table-against-FASTA validators (pangenomix_amd.pangenome.validate_table_against_fasta and its three
wrappers) without a device: the SHA-256 restatement of the reference (tests/dict_match_model.py) against what
the reference itself printed and raised (tests/golden/table_fasta), and the validators' own host work -- reading the files,
building the keys, naming, batching, the order of effects -- with the model's dictionary standing in for the device."""
import numpy as np
import pytest

import dict_match_model as model
from pangenomix_amd import pangenome as pg

CASES = model.load_cases()
TABLES = [(name, table) for name in sorted(CASES) for table in ('frame', 'lsdf') if table == 'frame' or model.is_binary(CASES[name])]
BATCHES = (None, 1)                       # TABLE_FASTA_BATCH_BYTES: the default, and one genome per call


def wrapper_of(case):
    return {'allele': pg.validate_allele_table, 'upstream': pg.validate_upstream_table,
            'downstream': pg.validate_downstream_table}[case['kind']]


@pytest.mark.parametrize('name', sorted(CASES))
def test_model_prints_and_raises_what_the_reference_did(name):
    case = CASES[name]
    genomes, nr, names = model.case_paths(case)
    out, exc = [], None
    try:
        model.validate(case['index'], case['columns'], model.case_cells(case), genomes, nr, names, case['log_group'], out=out)
    except (KeyError, FileNotFoundError) as e:
        exc = e
    assert ''.join(out).replace(model.GOLDEN, '<golden>') == case['stdout']
    if case['exception'] is None:
        assert exc is None
    else:
        assert type(exc).__name__ == case['exception']['type'] and exc.args[0] == case['exception']['arg']


def test_the_golden_cases_cover_what_they_should():
    assert len(CASES) >= 17
    assert sorted(str(c['exception']['arg']) for c in CASES.values() if c['exception']) == ['2', '2', 'q1b']
    out = {name: c['stdout'] for name, c in CASES.items()}
    assert out['cds_consistent'].endswith('Missing Features: 0\nFeature Table Inconsistencies: 0\n')
    assert 'gB \t Table only: 2 \t Genome only: 1\n' in out['cds_one_genome_differs']
    assert out['cds_several_genomes_differ'].count('Table only') == 3
    assert 'COLLISION: X_C2A0\nNon-redundant sequences: 6\n' in out['quirks']
    assert 'q1 \t Table only: 2 \t Genome only: 2\n' in out['quirks'] and 'q2 \t' not in out['quirks']
    assert out['quirks_genome_without_a_column'].endswith('q1 \t Table only: 2 \t Genome only: 2\nValidating genome 2 : '
                                                          '<golden>/table_fasta/quirks/q1b_x.faa\n')
    assert 'Validating genome 1' not in out['cds_unsorted_paths_log_group_2']
    assert 'g2 \t Table only: 0 \t Genome only: 1\n' in out['cds_frame_with_a_nan_and_a_2']
    assert 'gA \t Table only: 1 \t Genome only: 0\n' in out['cds_duplicate_index_labels']
    assert out['cds_no_genomes'].count('\n') == 4
    for side, letter in (('upstream', 'U'), ('downstream', 'D')):
        shared = out[side + '_shared_utrs_and_suffix_boundary']
        assert 'COLLISION: _C1%s0\nNon-redundant sequences: 4\n' % letter in shared
        assert 'u1 \t Table only: 1 \t Genome only: 1\n' in shared and 'u2 \t' not in shared
        assert 'p10 \t Table only: 1 \t Genome only: 1\n' in out[side + '_one_cell_flipped']
    assert any(c['other'] for c in CASES.values()) and any(len(set(c['index'])) < len(c['index']) for c in CASES.values())


@pytest.mark.parametrize('batch', BATCHES)
@pytest.mark.parametrize('name,table', TABLES)
def test_validators_with_the_model_dictionary_equal_the_reference(name, table, batch, capsys, monkeypatch):
    case = CASES[name]
    if batch is not None:
        monkeypatch.setattr(pg, 'TABLE_FASTA_BATCH_BYTES', batch)
    results = []
    for fn in (wrapper_of(case), pg.validate_table_against_fasta):
        ctx = model.ModelContext()
        df = model.case_frame(case) if table == 'frame' else model.case_lsdf(case)
        printed, result, exc = model.run_validator(fn, case, df, capsys, ctx=ctx)
        model.assert_as_recorded(case, printed, result, exc)
        results.append((printed, result, type(exc)))
        assert ctx.loads == 1 and ctx.diffs == (1 if 'Validating genome' in printed or 'Table only' in printed else 0)
        if batch == 1:
            assert len(ctx.queries) <= len(case['genomes'])                 # one genome per call (none for an empty one)
        elif ctx.queries:
            assert len(ctx.queries) == 1
    assert results[0] == results[1]


def test_one_genome_per_call_when_the_batch_is_one_byte(capsys, monkeypatch):
    case = CASES['cds_consistent']
    monkeypatch.setattr(pg, 'TABLE_FASTA_BATCH_BYTES', 1)
    ctx = model.ModelContext()
    model.run_validator(pg.validate_allele_table, case, model.case_lsdf(case), capsys, ctx=ctx)
    assert len(ctx.queries) == 6 and all(0 < q <= 49 for q in ctx.queries)       # (49 headers per genome file)
    monkeypatch.setattr(pg, 'TABLE_FASTA_BATCH_BYTES', 256 << 20)
    ctx = model.ModelContext()
    model.run_validator(pg.validate_allele_table, case, model.case_lsdf(case), capsys, ctx=ctx)
    assert len(ctx.queries) == 1


def test_tables_from_paths(tmp_path, capsys):
    """.npz is an LSDF, .csv goes through load_feature_table"""
    from pangenomix_amd import sparse_utils
    case = CASES['cds_one_genome_differs']
    model.case_frame(case).to_csv(str(tmp_path / 't.csv'))
    sparse_utils.LightSparseDataFrame.to_npz(model.case_lsdf(case), str(tmp_path / 't.npz'))
    for path in ('t.csv', 't.npz'):
        printed, result, exc = model.run_validator(pg.validate_allele_table, case, str(tmp_path / path), capsys,
                                                   ctx=model.ModelContext())
        model.assert_as_recorded(case, printed, result, exc)


RECORDS = {
    b'': ([], []),
    b'\n': ([''], [b'']),
    b'ACG': ([''], [b'ACG']),
    b'ACG\n': ([''], [b'ACG']),
    b'>h': ([], []),
    b'>h\n': ([], []),
    b'>h\n\n': (['h'], [b'']),
    b'>h\nAC\nGT': (['h'], [b'ACGT']),
    b'>h\nAC\nGT\n': (['h'], [b'ACGT']),
    b'>h\nAC\n\nGT\n\n': (['h'], [b'ACGT']),
    b'\n>h\nA': (['', 'h'], [b'', b'A']),
    b'>a\n>b\nX\n>c\n>d\n\n>e': (['b', 'd'], [b'X', b'']),
    b'>  a b\tc  \n  A C \n\tG\n': (['a b\tc'], [b'A CG']),
    b'>a>b\nA>C\n>c\n >d\n': (['a>b', 'c'], [b'A>C', b'>d']),
    b'>a\r\nAC\r\nGT\r\n>b\rTT\r': (['a', 'b'], [b'ACGT', b'TT']),              # universal newlines
    b'>a \x1c\nAC\x1f\n\x1dGT\n': (['a'], [b'ACGT']),                             # separators only str.strip() strips
    '>né \nAC \n GTé\n'.encode('utf-8'): (['né'], ['ACGTé'.encode('utf-8')]),
    b'>a\n\x0bAC\x0c\n G T \n': (['a'], [b'ACG T']),
}


@pytest.mark.parametrize('i', range(len(RECORDS)))
def test_fasta_records_are_what_text_mode_and_strip_give(i, tmp_path):
    data, want = list(RECORDS.items())[i]
    path = str(tmp_path / 'x.fa')
    with open(path, 'wb') as f:
        f.write(data)
    assert pg._fasta_records(path) == want
    assert pg._fasta_records_text(path) == want
    # and the statement-by-statement reading of the reference
    got_h, got_s = [], []
    header, blocks = '', []
    for line in open(path, 'r'):
        if line[0] == '>':
            if len(blocks) > 0:
                got_h.append(header)
                got_s.append(''.join(blocks).encode('utf-8'))
            header, blocks = line[1:].strip(), []
        else:
            blocks.append(line.strip())
    if len(blocks) > 0:
        got_h.append(header)
        got_s.append(''.join(blocks).encode('utf-8'))
    assert (got_h, got_s) == want


def test_feature_names_file(tmp_path):
    (tmp_path / 'n.tsv').write_text('A_C1A0\tfig|g.peg.1|tag\tf2\n  A_C2A0\tf3\tfig|g.peg.2  \nA_C3A0\nA_C4A0\tf2\ta|b|c|d\n')
    got = pg._feature_to_allele(str(tmp_path / 'n.tsv'))
    assert got == {'fig|g.peg.1': 'A_C1A0', 'f2': 'A_C4A0', 'f3': 'A_C2A0', 'fig|g.peg.2': 'A_C2A0', 'a|b|c|d': 'A_C4A0'}


def test_cells_equal_to_one():
    import pandas as pd
    nan = float('nan')
    df = pd.DataFrame([[1, 0, 2], [nan, 1.0, -1], [True, 1, 0.999]], index=['a', 'b', 'a'], columns=['x', 'y', 'z'])
    rows, cols, labels, columns = pg._cells_equal_to_one(df, 'who')
    assert sorted(zip(rows.tolist(), cols.tolist())) == [(0, 0), (1, 1), (2, 0), (2, 1)]
    assert labels.tolist() == ['a', 'b', 'a'] and columns.tolist() == ['x', 'y', 'z']
    assert rows.dtype == np.int32 and cols.dtype == np.int32
    with pytest.raises(TypeError):
        pg._cells_equal_to_one([[1]], 'who')
    # the rule of _table_cells is unchanged for its callers: a 2 in a frame is still refused there
    with pytest.raises(ValueError, match='binary'):
        pg._table_cells(df, 'who', notna=False)


def test_model_dictionary():
    keys = [b'', b'A', b'AB', b'A', b'', b'\x00', b'A\x00', b'A']
    first, last = model.first_last(keys, [b'A', b'', b'B', b'AB', b'\x00\x00'])
    assert first.tolist() == [0, 1, 2, 1, 0, 5, 6, 1] and last.tolist() == [7, 4, -1, 2, -1]
    data, offsets = model.blob(keys, lead=3)
    assert offsets[0] == 3 and model.strings_of(data, offsets) == keys
    a_only, b_only = model.sets_diff([0, 0, 1, 5], [0, 0, 1, 1], [0, 2, 5], [0, 0, 1], 6, 3)
    assert a_only.tolist() == [0, 1, 0] and b_only.tolist() == [1, 0, 0]
