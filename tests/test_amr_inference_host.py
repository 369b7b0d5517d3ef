"""pangenomix_amd.amr_inference without a device: ctx=None against what the reference returned and printed
(tests/golden/amr_inference), the Python 2 rules the reference cannot record under Python 3 against expectations written by
hand, infer_sir_batch against the loop over infer_sir, and the whole device path -- encoding, decoding, the hand-over of
irregular input -- through a stand-in context backed by the models of tests/mic_model.py."""
import numpy as np
import pandas as pd
import pytest

import amr_inference_cases as cases
import mic_model as model
from pangenomix_amd import amr_inference as ai

EXPECTED = cases.EXPECTED


@pytest.fixture(scope='module')
def table():
    return cases.golden_table()


@pytest.fixture(scope='module')
def generated():
    return model.generated_table()


# ---- ctx=None against the reference ---------------------------------------------------------------------------------------------
def test_constants_are_the_references():
    assert ai.NULL_TESTING_STANDARDS == {'missing'} and len(ai.ACCEPTED_MIC_METHODS) == 11
    assert np.nan in ai.MIC_EQUALITY_SIGNS and float('nan') not in ai.MIC_EQUALITY_SIGNS
    assert ai.MIC_INEQUALITY_SIGNS == {'>', '>=', '<', '<='}
    assert ai.MIC_BOUNDING_CASES == [('susceptible', {'<', '<='}), ('resistant', {'>', '>='})]


def test_primary_standards_are_the_references(table):
    got = ai.extract_primary_stnds(cases.ORG_TO_GIDS, table, cases.MIN_ENTRIES)
    assert cases.plain_frame(got.sort_index()) == EXPECTED['primary_stnds']


def test_mic_calls_are_the_references(table):
    got = ai.extract_mic_calls(cases.ORG_TO_GIDS, table, cases.MIN_ENTRIES)
    assert cases.plain_frame(got) == EXPECTED['mic_calls']
    assert got['mic_sign'].isin(['=', '==']).sum() == 0 and (got['count'] > 1).any()


def test_mappings_and_what_the_validator_prints_are_the_references(table, capsys):
    calls = ai.extract_mic_calls(cases.ORG_TO_GIDS, table, cases.MIN_ENTRIES)
    stnds = ai.extract_primary_stnds(cases.ORG_TO_GIDS, table, cases.MIN_ENTRIES).top_stnd
    ref_calls, ranges = ai.extract_mic_sir_mappings(calls, stnds, cases.MINIMUM_CALLS, allowed_sirs=EXPECTED['sir_order'])
    assert cases.plain(ref_calls) == EXPECTED['mic_ref_calls']
    assert cases.plain(ranges) == EXPECTED['mic_ranges']
    default_calls, default_ranges = ai.extract_mic_sir_mappings(calls, stnds, cases.MINIMUM_CALLS)
    assert default_calls == ref_calls and default_ranges == ranges       # (as dicts: whatever order the set iterates in)
    capsys.readouterr()
    ai.validate_mic_sir_mappings(ref_calls, ranges)
    printed = capsys.readouterr().out
    assert printed == EXPECTED['validate_printed']
    assert all(word in printed for word in ('AMBIGUOUS MIC-SIR:\t', 'INCONSISTENT S vs I:\t', 'INCONSISTENT S vs R:\t',
                                            'INCONSISTENT I vs R:\t', 'COMBINATION THERAPY:\t'))


def test_inference_is_the_references():
    ranges, stnds, columns = cases.golden_inference()
    got = [ai.infer_sir(*row, ranges, stnds) for row in zip(*columns)]
    assert cases.plain(got) == EXPECTED['inferred']
    assert {s for s, _ in got if isinstance(s, str)} == {'susceptible', 'intermediate', 'resistant'}


# ---- the quirks, by hand ------------------------------------------------------------------------------------------------------
STNDS = pd.Series({'o|d': 'clsi', 'o|a_b': 'clsi', 'o|polymyxin_b': 'clsi'}, dtype=object)


def test_the_order_of_the_classes_decides_where_ranges_overlap():
    s_first = {('o', 'd', 'clsi'): {'susceptible': [1.0, 4.0], 'intermediate': [4.0, 8.0], 'resistant': [8.0, 16.0]}}
    r_first = {('o', 'd', 'clsi'): {'resistant': [8.0, 16.0], 'intermediate': [4.0, 8.0], 'susceptible': [1.0, 4.0]}}
    assert ai.infer_sir('o', 'd', '8', np.nan, s_first, STNDS) == ('intermediate', 'clsi')
    assert ai.infer_sir('o', 'd', '8', np.nan, r_first, STNDS) == ('resistant', 'clsi')
    # a range hit of an earlier class beats a membership hit of a later one: 8.0 was observed as resistant
    assert ai.infer_sir('o', 'd', 8.0, '=', s_first, STNDS) == ('intermediate', 'clsi')
    assert ai.infer_sir('o', 'd', '0.01', '==', s_first, STNDS) == ('susceptible', 'clsi')     # open below
    assert ai.infer_sir('o', 'd', '900', np.nan, s_first, STNDS) == ('resistant', 'clsi')      # open above
    assert ai.infer_sir('o', 'd', '0.01', '<', s_first, STNDS)[0] == 'susceptible'             # '<' asks 'susceptible' alone
    assert ai.infer_sir('o', 'd', '6', '<=', s_first, STNDS)[0] is np.nan                      # above every susceptible MIC
    assert ai.infer_sir('o', 'd', '900', '>=', s_first, STNDS)[0] == 'resistant'
    assert ai.infer_sir('o', 'd', '6', '>', s_first, STNDS)[0] is np.nan


def test_signs_strings_and_what_raises():
    ranges = {('o', 'd', 'clsi'): {'intermediate': [4.0, 8.0]}, ('o', 'a_b', 'clsi'): {'susceptible': ['2/1'], 'resistant': ['8/4', 9.0]},
              ('o', 'polymyxin_b', 'clsi'): {'resistant': ['8/4', 9.0]}}
    nothing = lambda got: got[0] is np.nan and got[1] is np.nan
    assert nothing(ai.infer_sir('o', 'd', '6', float('nan'), ranges, STNDS))                   # another NaN is in neither set
    assert nothing(ai.infer_sir('o', 'd', '6', 'x', ranges, STNDS)) and nothing(ai.infer_sir('o', 'd', '6', None, ranges, STNDS))
    assert nothing(ai.infer_sir('o', 'd', '6', '<', ranges, STNDS))                            # no 'susceptible' class
    assert nothing(ai.infer_sir('x', 'd', '6', np.nan, ranges, STNDS))
    assert ai.infer_sir('o', 'd', '6', np.nan, ranges, STNDS) == ('intermediate', 'clsi')
    assert nothing(ai.infer_sir('o', 'd', '9', np.nan, ranges, STNDS))
    assert ai.infer_sir('o', 'a_b', '8/4', np.nan, ranges, STNDS) == ('resistant', 'clsi')
    assert nothing(ai.infer_sir('o', 'a_b', '9', np.nan, ranges, STNDS))                       # '9' is not 9.0, and no range test
    assert ai.infer_sir('o', 'a_b', 9.0, np.nan, ranges, STNDS) == ('resistant', 'clsi')
    assert ai.infer_sir('o', 'a_b', '2/1', '<=', ranges, STNDS) == ('susceptible', 'clsi')
    with pytest.raises(TypeError):                                                             # min() over a float and a str
        ai.infer_sir('o', 'polymyxin_b', '3', np.nan, ranges, STNDS)
    with pytest.raises(TypeError):
        ai.infer_sir('o', 'd', None, np.nan, ranges, STNDS)
    assert ai.__is_combination_therapy__('a_b') and not ai.__is_combination_therapy__('nalidixic_acid')
    assert not ai.__is_combination_therapy__('polymyxin_b') and not ai.__is_combination_therapy__('ampicillin')


def test_equals_four_is_not_numeric_so_the_row_is_a_likely_combination():
    """float('=4') raises ValueError inside the try: the MIC is taken as not numeric, and no range test follows"""
    ranges = {('o', 'd', 'clsi'): {'intermediate': [4.0, 8.0]}}
    got = ai.infer_sir('o', 'd', '=4', np.nan, ranges, STNDS)
    assert got[0] is np.nan and got[1] is np.nan


def test_a_reported_mic_with_an_equals_sign_raises_in_the_mappings():
    """'=4' has no slash, so extract_mic_sir_mappings calls float('=4'): ValueError, as in the reference"""
    calls = pd.DataFrame([['o', 'd', 'clsi', 'resistant', '=4', np.nan, '4', 5]],
                         columns=['organism', 'drug', 'standard', 'sir', 'mic', 'mic_sign', 'mic_val', 'count'])
    with pytest.raises(ValueError):
        ai.extract_mic_sir_mappings(calls, STNDS)
    calls['mic'] = '4'
    assert ai.extract_mic_sir_mappings(calls, STNDS)[1] == {('o', 'd', 'clsi'): {'resistant': [4.0]}}


def small_table(rows):
    """rows of (genome, drug, sir, mic, sign, standard): mg/L and a MIC method throughout"""
    data = [[g, 'n', '1', d, sir, mic, sign, mic, 'mg/L', 'etest', None, None, None, stnd, None, None, None, 's']
            for g, d, sir, mic, sign, stnd in rows]
    df = pd.DataFrame(data, columns=model.PATRIC_COLUMNS)
    for col in ('resistant_phenotype', 'measurement_sign', 'testing_standard'):      # every null is the np.nan object, as
        values = np.empty(len(df), dtype=object)                                     # read_csv leaves it in an object column
        values[:] = [np.nan if pd.isnull(v) else v for v in df[col].tolist()]
        df[col] = values
    return df


@pytest.mark.parametrize('ctx', (None, 'stand-in'))
def test_a_null_sorts_before_every_string_as_under_python_2(ctx):
    ctx = model.StandIn() if ctx else None
    df = small_table([('g1', 'd', 'resistant', '2', '<', 'clsi'), ('g1', 'd', 'resistant', '2', np.nan, 'clsi'),
                      ('g1', 'd', np.nan, '2', np.nan, 'clsi'), ('g1', 'd', 'intermediate', '2', '=', 'clsi'),
                      ('g1', 'd', 'resistant', '2', '==', np.nan), ('g1', 'd', 'resistant', '2', '=', 'clsi'),
                      ('g1', 'd', 'resistant', '1', '>', 'bsac'), ('g1', 'd', 'resistant', '2', np.nan, 'missing')])
    got = ai.extract_mic_calls({'o': ['g1']}, df, 1, ctx=ctx)
    rows = [tuple(None if (isinstance(v, float) and v != v) else v for v in r) for r in got.values.tolist()]
    assert rows == [('o', 'd', None, 'resistant', '2', None, '2', 1),
                    ('o', 'd', 'bsac', 'resistant', '1', '>', '1', 1),
                    ('o', 'd', 'clsi', None, '2', None, '2', 1),
                    ('o', 'd', 'clsi', 'intermediate', '2', None, '2', 1),
                    ('o', 'd', 'clsi', 'resistant', '2', None, '2', 2),
                    ('o', 'd', 'clsi', 'resistant', '2', '<', '2', 1)]


@pytest.mark.parametrize('ctx', (None, 'stand-in'))
def test_other_standards_have_the_python_2_meaning_of_filter(ctx):
    ctx = model.StandIn() if ctx else None
    rows = [('g1', 'd', 'resistant', '2', np.nan, s) for s in ['clsi'] * 5 + [np.nan] * 7 + ['eucast'] * 3 + ['bsac'] * 2]
    rows += [('g2', 'e', 'resistant', '2', np.nan, np.nan)] * 3 + [('g2', 'f', 'resistant', '2', np.nan, 'clsi')] * 2
    rows += [('g2', 'one', 'resistant', '2', np.nan, 'clsi')]
    got = ai.extract_primary_stnds({'o': ['g1', 'g2']}, small_table(rows), 2, ctx=ctx).sort_index()
    assert got.index.tolist() == ['o|d', 'o|e', 'o|f']
    assert got.loc['o|d'].tolist() == ['clsi', 5, 5, 7, 'eucast;bsac']
    assert got.loc['o|f'].tolist()[:4] == ['clsi', 2, 0, 0] and pd.isnull(got.loc['o|f', 'other_stnds'])
    e = got.loc['o|e']
    assert pd.isnull(e.top_stnd) and pd.isnull(e.other_stnds) and (e.n_top_stnd, e.n_other_stnd, e.n_missing_stnd) == (3, 0, 3)


# ---- infer_sir_batch --------------------------------------------------------------------------------------------------------------
SIGNS = [np.nan, float('nan'), '=', '==', '<', '<=', '>', '>=', 'x', None]


def batch_columns(values):
    n = len(SIGNS) * len(values)
    signs = np.empty(n, dtype=object)
    signs[:] = SIGNS * len(values)
    vals = np.empty(n, dtype=object)
    vals[:] = [v for v in values for _ in SIGNS]
    orgs = np.array(['o'] * n, dtype=object)
    drugs = np.array((['d', 'a_b', 'polymyxin_b', 'unknown'] * n)[:n], dtype=object)
    return orgs, drugs, vals, signs


RANGES = {('o', 'd', 'clsi'): {'susceptible': [1.0, 4.0], 'intermediate': [4.0, 8.0], 'resistant': [8.0, 16.0]},
          ('o', 'a_b', 'clsi'): {'resistant': ['8/4', '16/8'], 'susceptible': ['2/1']},
          ('o', 'polymyxin_b', 'clsi'): {'intermediate': [2.0], 'resistant': [4.0, 8.0]}}


@pytest.mark.parametrize('ctx', (None, 'stand-in'))
def test_batch_is_the_loop_on_every_sign(ctx):
    ctx = model.StandIn() if ctx else None
    columns = batch_columns(['0.5', '4', '4.0', 4.0, '8', 8.0, 6.5, '32', float('nan'), '8/4', '2/1', 'n/a', float('inf')])
    want = [ai.infer_sir(*row, RANGES, STNDS) for row in zip(*columns)]
    before = cases.counts()
    sir, stnd = ai.infer_sir_batch(*columns, RANGES, STNDS, ctx=ctx)
    assert cases.path_of(before, 'infer_sir_batch') == ('device' if ctx else 'host')
    assert sir.dtype == object and stnd.dtype == object
    for i, (s, t) in enumerate(want):
        assert (sir[i] is s or sir[i] == s) and (stnd[i] is t or stnd[i] == t), i
    hits = [s for s in sir.tolist() if isinstance(s, str)]
    assert {'susceptible', 'intermediate', 'resistant'} == set(hits) and len(hits) < sir.size
    assert sir[1] is np.nan                               # float('nan') as a sign: in neither set


@pytest.mark.parametrize('ctx', (None, 'stand-in'))
def test_batch_raises_what_the_first_raising_row_raises(ctx):
    ctx = model.StandIn() if ctx else None
    orgs, drugs, vals, signs = batch_columns(['4', '8'])
    vals[7], vals[9] = None, [1]                          # float(None) raises TypeError before float([1]) does
    with pytest.raises(TypeError, match='NoneType'):
        ai.infer_sir_batch(orgs, drugs, vals, signs, RANGES, STNDS, ctx=ctx)
    mixed = dict(RANGES)
    mixed[('o', 'polymyxin_b', 'clsi')] = {'resistant': [4.0, '8/4']}
    orgs, drugs, vals, signs = batch_columns(['4'])
    before = cases.counts()
    with pytest.raises(TypeError):
        ai.infer_sir_batch(orgs, drugs, vals, signs, mixed, STNDS, ctx=ctx)
    assert cases.path_of(before, 'infer_sir_batch') == 'host'
    with pytest.raises(ValueError):
        ai.infer_sir_batch(orgs[:3], drugs, vals, signs, RANGES, STNDS, ctx=ctx)
    empty = ai.infer_sir_batch([], [], [], [], RANGES, STNDS, ctx=ctx)
    assert empty[0].shape == (0,) and empty[1].dtype == object


# ---- the device path through the stand-in -------------------------------------------------------------------------------------------
def test_device_path_on_the_golden_table(table):
    ctx = model.StandIn()
    want = cases.check_extractors(ctx, cases.ORG_TO_GIDS, table, cases.MIN_ENTRIES, 'device')
    assert cases.plain_frame(want[1]) == EXPECTED['mic_calls']
    assert ctx.calls['tuple_group'] == 4
    ranges, stnds, columns = cases.golden_inference()
    want = cases.check_batch(ctx, columns, ranges, stnds, 'device')
    assert cases.plain(list(zip(*[w.tolist() for w in want[1]]))) == EXPECTED['inferred']
    assert ctx.calls['mic_infer'] == 1


@pytest.mark.parametrize('min_entries', (20, 100, 10 ** 6))
@pytest.mark.parametrize('stnd_col', ('testing_standard', 'laboratory_typing_platform', 'testing_standard_year'))
def test_device_path_on_a_generated_table_with_ties_and_nulls(generated, min_entries, stnd_col):
    org_to_gids, df = generated
    if stnd_col == 'testing_standard_year':               # (a float column without a NaN is a regular key column)
        assert df[stnd_col].dtype == np.float64
    want = cases.check_extractors(model.StandIn(), org_to_gids, df, min_entries, 'device', stnd_col=stnd_col)
    if min_entries == 20:
        calls = want[1]
        assert calls['count'].max() > 1 and pd.isnull(calls['standard']).any() and pd.isnull(calls['sir']).any()


def test_ties_between_counts_are_pandas_own(generated):
    """standards with equal counts, and a null among them, in every first-appearance order"""
    import itertools
    for order in itertools.permutations(['clsi', 'eucast', np.nan]):
        rows = [('g1', 'd', 'resistant', '2', np.nan, s) for s in list(order) * 2 + ['bsac']]
        cases.check_extractors(model.StandIn(), {'o': ['g1']}, small_table(rows), 1, 'device')


def test_device_path_of_the_batch_on_a_generated_table(generated):
    org_to_gids, df = generated
    ranges, stnds, columns = model.inference_inputs(org_to_gids, df, 20)
    assert len(ranges) >= 3
    want = cases.check_batch(model.StandIn(), columns, ranges, stnds, 'device')
    assert want[0] == 'returned' and len({s for s in want[1][0].tolist() if isinstance(s, str)}) == 3


@pytest.mark.parametrize('name,change,functions', cases.IRREGULAR_TABLES, ids=[c[0] for c in cases.IRREGULAR_TABLES])
def test_irregular_tables_go_to_the_host(table, name, change, functions):
    cases.check_irregular_table(model.StandIn(), name, change, functions, cases.ORG_TO_GIDS, table, cases.MIN_ENTRIES)


def test_irregular_batches_go_to_the_host():
    ranges, stnds, columns = cases.golden_inference()
    cases.check_irregular_batches(model.StandIn(), ranges, stnds, columns)


def test_sizes_past_the_limits_go_to_the_host(table, monkeypatch):
    monkeypatch.setattr(ai, '_TUPLE_MAX_ROWS', 50)
    cases.check_extractors(model.StandIn(), cases.ORG_TO_GIDS, table, cases.MIN_ENTRIES, 'host')
    ranges, stnds, columns = cases.golden_inference()
    monkeypatch.setattr(ai, '_MIC_MAX_ROWS', 50)
    cases.check_batch(model.StandIn(), columns, ranges, stnds, 'host')
    monkeypatch.setattr(ai, '_MIC_MAX_ROWS', 1 << 31)
    monkeypatch.setattr(ai, '_MIC_MAX_TABLE', 3)
    cases.check_batch(model.StandIn(), columns, ranges, stnds, 'host')
