"""pangenomix_amd.amr_inference with a device context against ctx=None in one process: frames equal under
assert_frame_equal with dtypes, object arrays equal element by element, and AMR_INFERENCE_PATH_COUNTS naming the path --
"device" for regular input, "host" for each irregular one. Strings and integers: nothing here is approximate."""
import pytest

import amr_inference_cases as cases
import mic_model as model
from pangenomix_amd import amr_inference as ai

pytestmark = pytest.mark.gpu

EXPECTED = cases.EXPECTED


@pytest.fixture(scope='module')
def table():
    return cases.golden_table()


@pytest.fixture(scope='module')
def generated():
    return model.generated_table()


def test_extractors_on_the_golden_table(table, gpu_ctx):
    want = cases.check_extractors(gpu_ctx, cases.ORG_TO_GIDS, table, cases.MIN_ENTRIES, 'device')
    assert cases.plain_frame(want[1]) == EXPECTED['mic_calls']
    stnds = ai.extract_primary_stnds(cases.ORG_TO_GIDS, table, cases.MIN_ENTRIES, ctx=gpu_ctx)
    assert cases.plain_frame(stnds.sort_index()) == EXPECTED['primary_stnds']


def test_batch_on_the_golden_table(gpu_ctx):
    ranges, stnds, columns = cases.golden_inference()
    want = cases.check_batch(gpu_ctx, columns, ranges, stnds, 'device')
    assert cases.plain(list(zip(*[w.tolist() for w in want[1]]))) == EXPECTED['inferred']


@pytest.mark.parametrize('min_entries', (20, 100))
@pytest.mark.parametrize('stnd_col', ('testing_standard', 'testing_standard_year'))
def test_extractors_on_a_generated_table_with_ties_and_nulls(generated, min_entries, stnd_col, gpu_ctx):
    org_to_gids, df = generated
    want = cases.check_extractors(gpu_ctx, org_to_gids, df, min_entries, 'device', stnd_col=stnd_col)
    assert len(want[1]) > 100 and want[1]['count'].max() > 1


def test_batch_on_a_generated_table(generated, gpu_ctx):
    org_to_gids, df = generated
    ranges, stnds, columns = model.inference_inputs(org_to_gids, df, 20)
    want = cases.check_batch(gpu_ctx, columns, ranges, stnds, 'device')
    assert want[0] == 'returned' and len({s for s in want[1][0].tolist() if isinstance(s, str)}) == 3


@pytest.mark.parametrize('name,change,functions', cases.IRREGULAR_TABLES, ids=[c[0] for c in cases.IRREGULAR_TABLES])
def test_irregular_tables_go_to_the_host(table, name, change, functions, gpu_ctx):
    cases.check_irregular_table(gpu_ctx, name, change, functions, cases.ORG_TO_GIDS, table, cases.MIN_ENTRIES)


def test_irregular_batches_go_to_the_host(gpu_ctx):
    ranges, stnds, columns = cases.golden_inference()
    cases.check_irregular_batches(gpu_ctx, ranges, stnds, columns)


def test_sizes_past_the_limits_go_to_the_host(table, monkeypatch, gpu_ctx):
    monkeypatch.setattr(ai, '_TUPLE_MAX_ROWS', 50)
    cases.check_extractors(gpu_ctx, cases.ORG_TO_GIDS, table, cases.MIN_ENTRIES, 'host')
    ranges, stnds, columns = cases.golden_inference()
    monkeypatch.setattr(ai, '_MIC_MAX_TABLE', 3)
    cases.check_batch(gpu_ctx, columns, ranges, stnds, 'host')
