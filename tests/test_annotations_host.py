"""extract_annotations and generate_annotations without a GPU: the host path against every case the reference recorded
(tests/golden/annotations: file bytes, stdout, the exception, the .tmp files left behind), the ctx= layer on a model context
(the dictionary of tests/dict_match_model.py, the vote of tests/annot_model.py) against the same records and against the
host path, and the model of pgx_annot_vote against a collections formulation of what the reference's loops do."""
import collections

import numpy as np
import pytest

import annot_model as model
import annotations_cases as cases
import dict_match_model
from pangenomix_amd import _native, pangenome as pg


class ModelContext(dict_match_model.ModelContext):
    def __init__(self):
        super().__init__()
        self.votes = 0

    def annot_vote(self, tok, row_off, run_off, flags=0):
        self.votes += 1
        tok, row_off = np.asarray(tok).tolist(), [int(x) for x in row_off]
        assert all(x >= 0 for x in tok) and row_off[0] == 0 and int(run_off[0]) == 0 and int(run_off[-1]) == len(row_off) - 1
        assert (np.diff(np.asarray(run_off, dtype=np.int64)) > 0).all()
        return model.vote_fast([tok[row_off[r]:row_off[r + 1]] for r in range(len(row_off) - 1)], run_off)


# -- the host path -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', cases.EXTRACT_CASES)
def test_extract_annotations_host_path_equals_the_reference(case, tmp_path, capsys):
    pg.ANNOTATION_PATH_COUNTS.clear()
    cases.assert_recorded(case, cases.run_extract(case, tmp_path / 'w', capsys, ctx=None))
    assert dict(pg.ANNOTATION_PATH_COUNTS) == {'extract_host': 1}


@pytest.mark.parametrize('case', cases.GENERATE_CASES)
def test_generate_annotations_host_path_equals_the_reference(case, tmp_path):
    pg.ANNOTATION_PATH_COUNTS.clear()
    cases.assert_recorded(case, cases.run_generate(case, tmp_path, ctx=None))
    assert dict(pg.ANNOTATION_PATH_COUNTS) == {'generate_host': 1}


def test_the_recorded_cases_are_the_ones_the_paths_are_judged_by():
    regular = {c for c in cases.EXTRACT_CASES if cases.load_case(c)['regular']}
    assert {'two_gffs_batch100', 'two_gffs_batch1', 'collapse_false', 'flexible_locus_tag', 'allowed_trna', 'tie_first_seen',
            'single_gene', 'alleles_without_a', 'same_key_batch100', 'same_key_batch1'} <= regular
    assert {'tab_in_product', 'product_is_later_key_batch100', 'product_is_later_key_batch1', 'attribute_without_equals',
            'attribute_with_two_equals', 'blank_names_line', 'crlf', 'non_ascii_product'} == \
        {c for c in cases.EXTRACT_CASES if c not in regular} - {'empty_product'}
    # the quirks the fixtures are there for did happen in the reference's run
    out = lambda c: open(cases.os.path.join(cases.GOLDEN, c, 'expected.tsv')).read()   # noqa: E731
    assert out('single_gene') == '' and out('two_gffs_batch100').count('T_C0\t') == 2 and 'last_C5' not in out('two_gffs_batch100')
    assert out('tie_first_seen').startswith('T_C0\tPhage protein\n')
    assert out('same_key_batch100') != out('same_key_batch1')
    assert out('product_is_later_key_batch100') != out('product_is_later_key_batch1')


# -- the ctx= layer on a model context ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', cases.EXTRACT_CASES)
def test_extract_annotations_with_a_context_equals_the_reference_and_takes_the_right_path(case, tmp_path, capsys):
    ctx = ModelContext()
    pg.ANNOTATION_PATH_COUNTS.clear()
    got = cases.run_extract(case, tmp_path / 'w', capsys, ctx=ctx)
    cases.assert_recorded(case, got)
    regular = cases.load_case(case)['regular']
    assert dict(pg.ANNOTATION_PATH_COUNTS) == ({'extract_device': 1} if regular else {'extract_host': 1})
    assert ctx.votes == (1 if regular else 0)


@pytest.mark.parametrize('case', cases.GENERATE_CASES)
def test_generate_annotations_with_a_context_equals_the_reference(case, tmp_path):
    ctx = ModelContext()
    pg.ANNOTATION_PATH_COUNTS.clear()
    cases.assert_recorded(case, cases.run_generate(case, tmp_path, ctx=ctx))
    regular = cases.load_case(case)['regular']
    assert dict(pg.ANNOTATION_PATH_COUNTS) == ({'generate_device': 1} if regular else {'generate_host': 1})
    assert ctx.loads == (1 if regular else 0)


@pytest.mark.parametrize('kw', (dict(batch=100), dict(batch=2), dict(collapse_alleles=False), dict(flexible_locus_tag=True),
                                dict(allowed_features=['CDS', 'rRNA']), dict(allowed_features=[])))
def test_both_paths_agree_on_a_generated_set(kw, tmp_path, capsys):
    gffs, names = cases.generated_set(tmp_path, n_genomes=5, n_genes=120, big_run=70, big_row=80)
    out_h, out_d = str(tmp_path / 'h.tsv'), str(tmp_path / 'd.tsv')
    pg.extract_annotations(gffs, names, out_h, **kw)
    printed = capsys.readouterr().out
    pg.ANNOTATION_PATH_COUNTS.clear()
    pg.extract_annotations(gffs, names, out_d, ctx=ModelContext(), **kw)
    assert capsys.readouterr().out == printed and printed.count('Loaded') == (3 if kw.get('batch') == 2 else 1)
    assert dict(pg.ANNOTATION_PATH_COUNTS) == {'extract_device': 1}
    assert open(out_d, 'rb').read() == open(out_h, 'rb').read()
    assert not list(tmp_path.glob('*.tmp*'))


def test_odd_arguments_go_to_the_host(tmp_path, capsys):
    gffs, names = cases.generated_set(tmp_path, n_genomes=2, n_genes=10, big_run=2, big_row=1)
    for kw, error in ((dict(batch=0), ValueError), (dict(allowed_features='CDS_or_tRNA'), None), (dict(batch=1.5), TypeError)):
        pg.ANNOTATION_PATH_COUNTS.clear()
        if error is None:
            pg.extract_annotations(gffs, names, str(tmp_path / 'o.tsv'), ctx=ModelContext(), **kw)
        else:
            with pytest.raises(error):
                pg.extract_annotations(gffs, names, str(tmp_path / 'o.tsv'), ctx=ModelContext(), **kw)
        assert dict(pg.ANNOTATION_PATH_COUNTS) == {'extract_host': 1}
    pg.ANNOTATION_PATH_COUNTS.clear()
    with pytest.raises(FileNotFoundError):
        pg.extract_annotations(gffs + [str(tmp_path / 'missing.gff')], names, str(tmp_path / 'o.tsv'), ctx=ModelContext())
    assert dict(pg.ANNOTATION_PATH_COUNTS) == {'extract_host': 1}


# -- the model of the device step --------------------------------------------------------------------------------------------
def collections_vote(rows, run_off):
    """the reference's own tools: OrderedDict.fromkeys per row, Counter.most_common per run"""
    lists = [tuple(collections.OrderedDict.fromkeys(row)) for row in rows]
    keep = [1 if x not in row[:p] else 0 for row in rows for p, x in enumerate(row)]
    winner, votes, differs = [], [], [0] * len(rows)
    for u in range(len(run_off) - 1):
        members = list(range(int(run_off[u]), int(run_off[u + 1])))
        best, count = collections.Counter(lists[r] for r in members).most_common(1)[0]
        winner.append(next(r for r in members if lists[r] == best))
        votes.append(count)
        for r in members:
            differs[r] = int(lists[r] != best)
    return keep, winner, votes, differs


@pytest.mark.parametrize('seed', range(6))
def test_the_model_equals_the_collections_formulation(seed):
    rng = np.random.default_rng(seed)
    rows = [[int(x) for x in rng.integers(0, 4, int(k))] for k in rng.integers(0, 5, 400)]
    cuts = np.unique(np.concatenate(([0, len(rows)], rng.integers(0, len(rows), 60))))
    want = collections_vote(rows, cuts)
    for fn in (model.vote, model.vote_fast):
        got = fn(rows, cuts)
        assert [g.tolist() for g in got] == [list(w) for w in want]
        assert [str(g.dtype) for g in got] == ['uint8', 'int32', 'uint32', 'uint8']


# -- the ABI without a device ------------------------------------------------------------------------------------------------
def test_tiles_and_workspace_sizes_need_no_device():
    lib = _native.lib()
    assert lib.pgx_annot_row_tile() >= 16 and lib.pgx_annot_run_tile() >= 1
    assert lib.pgx_annot_vote_workspace_bytes(1 << 24, 0, 1) == 0            # sizes that are refused
    assert lib.pgx_annot_vote_workspace_bytes(10, 1 << 31, 1) == 0
    assert lib.pgx_annot_vote_workspace_bytes(10, 5, 11) == 0
    small, large = lib.pgx_annot_vote_workspace_bytes(10, 30, 4), lib.pgx_annot_vote_workspace_bytes(1000, 3000, 4)
    assert 0 < small < large and small % 256 == 0
    assert lib.pgx_annot_vote(None, None, None, 0, None, 0, 0, None, None, None, None) == -1   # a NULL context: PGX_ERR_INVALID
