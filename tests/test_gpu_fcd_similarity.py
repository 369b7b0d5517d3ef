"""Comparing two concept lists on the device (pangenomix_amd/fcd.py: compute_concept_list_similarity with a context,
match_concept_lists, concept_overlaps; csrc/fcd_match.hip) against the scores the reference produced
(tests/golden/fcd_similarity/scores.json) and, for the pairing and the matrix the reference throws away, against the numpy
model of the same rule (tests/fcd_similarity_model.py, itself checked against every score in
tests/test_fcd_similarity_host.py). Every comparison is exact."""
import json

import numpy as np
import pytest
import scipy.sparse

import dev_entry_checks as chk
import fcd_similarity_model as sim
from pangenomix_amd import _native, fcd, sparse_utils

pytestmark = pytest.mark.gpu

SCORES = json.load(open(sim.SCORES))


@pytest.mark.parametrize('name', sim.CASES)
def test_every_case_exactly(name, gpu_ctx):
    F1, F2, S = sim.case_inputs(name)
    want = sim.expected(name)
    if SCORES[name].startswith('0x'):
        assert fcd.compute_concept_list_similarity(F1, F2, S, ctx=gpu_ctx).hex() == SCORES[name]
    else:
        assert SCORES[name] == 'ZeroDivisionError'
        with pytest.raises(ZeroDivisionError):
            fcd.compute_concept_list_similarity(F1, F2, S, ctx=gpu_ctx)
    match, overlap, total = fcd.match_concept_lists(F1, F2, S.shape, ctx=gpu_ctx)
    assert match.dtype == np.int64 and overlap.dtype == np.int64 and type(total) is int
    assert np.array_equal(match, want['match']) and np.array_equal(overlap, want['overlap']) and total == want['total']
    O = fcd.concept_overlaps(F1, F2, S.shape, ctx=gpu_ctx)
    assert O.dtype == np.int64 and O.shape == (len(F1), len(F2)) and np.array_equal(O, want['O'])


def test_the_same_call_twice_gives_the_same_arrays(gpu_ctx):
    import torch
    F1, F2, S = sim.case_inputs('gen_65x400_257x130')
    first = fcd.match_concept_lists(F1, F2, S.shape, ctx=gpu_ctx)
    O = fcd.concept_overlaps(F1, F2, S.shape, ctx=gpu_ctx)
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info()[0]
    again = fcd.match_concept_lists(F1, F2, S.shape, ctx=gpu_ctx)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1]) and first[2] == again[2]
    assert np.array_equal(fcd.concept_overlaps(F1, F2, S.shape, ctx=gpu_ctx), O)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free_before                  # the workspace slots are reused


def test_a_decomposition_and_a_comparison_do_not_disturb_each_other(gpu_ctx):
    fx = sim.fixture('blocks_1500x90_overlap')
    other = sim.fixture('blocks_1500x90_seed_limit')['F']
    S = fx['dense']()
    name = 'blocks_1500x90_overlap__blocks_1500x90_seed_limit'
    for _ in range(2):
        F = fcd.formal_concept_decomposition(S, ctx=gpu_ctx, **fx['kwargs'])[2]
        assert [(list(x), list(y)) for x, y in F] == [(list(x), list(y)) for x, y in fx['F']]
        assert np.array_equal(fcd.compute_concept_coverage(S, F, log_rate=0, ctx=gpu_ctx), fx['coverage'])
        assert fcd.compute_concept_list_similarity(F, other, S, ctx=gpu_ctx).hex() == SCORES[name]


def test_indices_outside_the_table_raise_index_error(gpu_ctx):
    good = [((0, 2), (1,)), ((1, 2, 3), (0, 2))]
    S = np.ones((4, 3), dtype=int)
    for bad in ([((4,), (0,))], [((0,), (3,))], [((-1,), (0,))], [((0,), (-1,))]):
        for F1, F2 in ((bad, good), (good, bad)):
            with pytest.raises(IndexError):
                fcd.compute_concept_list_similarity(F1, F2, S, ctx=gpu_ctx)
            with pytest.raises(IndexError):
                fcd.match_concept_lists(F1, F2, S.shape, ctx=gpu_ctx)
    # the last valid indices, listed twice: accepted, and counted once
    edge = [((3, 3, 0), (2, 2))]
    assert fcd.match_concept_lists(edge, edge, S.shape, ctx=gpu_ctx)[2] == 2


def test_the_library_checks_what_it_is_given(gpu_ctx):
    i32, u64 = (lambda *v: np.array(v, dtype=np.int32)), (lambda *v: np.array(v, dtype=np.uint64))
    one = (i32(0), u64(0, 1), i32(0), u64(0, 1))
    assert gpu_ctx.fcd_match(4, 4, *(one + one))[2] == 1
    with pytest.raises(_native.PgxError, match='out of range'):
        gpu_ctx.fcd_match(4, 4, *(one + (i32(4), u64(0, 1), i32(0), u64(0, 1))))
    with pytest.raises(_native.PgxError, match='out of range'):
        gpu_ctx.fcd_match(4, 4, *((i32(0), u64(0, 1), i32(-1), u64(0, 1)) + one))
    with pytest.raises(_native.PgxError, match='offsets'):
        gpu_ctx.fcd_match(4, 4, *((i32(0, 1, 2), u64(0, 2, 1, 3), i32(0, 0, 0), u64(0, 1, 2, 3)) + one))
    with pytest.raises(_native.PgxError, match='too large'):
        gpu_ctx.fcd_match(2 ** 31, 4, *(one + one))
    three = (i32(0, 0, 0), u64(0, 1, 2, 3), i32(0, 0, 0), u64(0, 1, 2, 3))
    with pytest.raises(_native.PgxError, match='63 bits'):               # (2^31 - 1)^2 * 3 >= 2^63; * 2 still fits
        gpu_ctx.fcd_match(2 ** 31 - 1, 2 ** 31 - 1, *(three + three))
    assert gpu_ctx.fcd_match_workspace_bytes(2 ** 31, 4, 1, 1) == 0
    none = (i32(), u64(0), i32(), u64(0))
    match, overlap, total, O = gpu_ctx.fcd_match(4, 4, *(none + one), matrix=True)
    assert match.size == 0 and overlap.size == 0 and total == 0 and O.shape == (0, 1)


def test_sparse_tables_give_the_dense_score(gpu_ctx):
    fx = sim.fixture('rows_193')
    F1, F2 = fx['F'], sim.fixture('rows_193_seed')['F']
    S = fx['dense']()
    coo = scipy.sparse.coo_matrix((np.ones(fx['rows'].size, dtype=np.int64), (fx['rows'], fx['cols'])), shape=fx['shape'])
    lsdf = sparse_utils.LightSparseDataFrame(['r%d' % i for i in range(fx['shape'][0])],
                                             ['c%d' % j for j in range(fx['shape'][1])], coo)
    want = SCORES['rows_193__rows_193_seed']
    for X in (S, coo, coo.tocsr(), lsdf):
        assert fcd.compute_concept_list_similarity(F1, F2, X, ctx=gpu_ctx).hex() == want


# ---- pgx_fcd_match_dev: caller tensors, caller stream (tests/dev_entry_checks.py) ------------------------------------------
DEV_CASES = ('gen_65x400_257x130', 'gen_70001x65_3x70', 'blocks_3000x120_dim_balance__blocks_3000x120')


def dev_masks(name):
    F1, F2, S = sim.case_inputs(name)
    n_rows, n_cols = S.shape
    lib = _native.lib()
    sr, sc = int(lib.pgx_bitmap_stride_words(n_rows)), int(lib.pgx_bitmap_stride_words(n_cols))
    masks = (sim.pack([f[0] for f in F1], n_rows, sr), sim.pack([f[1] for f in F1], n_cols, sc),
             sim.pack([f[0] for f in F2], n_rows, sr), sim.pack([f[1] for f in F2], n_cols, sc))
    return masks, len(F1), len(F2), n_rows, n_cols


def run_match_dev(ctx, kind, fill, masks, n1, n2, n_rows, n_cols, with_matrix):
    k = min(n1, n2)
    nws = ctx.fcd_match_workspace_bytes(n_rows, n_cols, n1, n2)
    with chk.stream_scope(kind) as st:
        ws = chk.guarded(nws, fill)
        outs = [chk.guarded(k * 8, fill), chk.guarded(k * 8, fill), chk.guarded(8, fill)]
        if with_matrix:
            outs.append(chk.guarded(n1 * n2 * 8, fill))
        ups = [chk.upload(m) for m in masks]
        with chk.unchanged(*ups):
            ctx.fcd_match_dev(ups[0].ptr, ups[1].ptr, n1, ups[2].ptr, ups[3].ptr, n2, n_rows, n_cols, outs[0].ptr, outs[1].ptr,
                              outs[2].ptr, ws.ptr, nws, d_matrix=outs[3].ptr if with_matrix else None, stream=st)
    for g in outs + [ws]:
        g.assert_guards_intact()
    got = (outs[0].numpy(np.int64), outs[1].numpy(np.uint64), outs[2].numpy(np.uint64))
    return got + ((outs[3].numpy(np.uint64).reshape(n1, n2),) if with_matrix else ())


@pytest.mark.parametrize('with_matrix', [True, False], ids=['matrix', 'no_matrix'])
@pytest.mark.parametrize('kind', chk.STREAMS)
@pytest.mark.parametrize('name', DEV_CASES)
def test_fcd_match_dev_on_caller_tensors(name, kind, with_matrix, gpu_ctx):
    masks, n1, n2, n_rows, n_cols = dev_masks(name)
    want = sim.expected(name)
    got = chk.same_bytes([run_match_dev(gpu_ctx, kind, f, masks, n1, n2, n_rows, n_cols, with_matrix) for f in chk.FILLS])
    assert np.array_equal(got[0], want['match']) and np.array_equal(got[1].astype(np.int64), want['overlap'])
    assert int(got[2][0]) == want['total']
    if with_matrix:
        assert np.array_equal(got[3].astype(np.int64), want['O'])
    F1, F2, S = sim.case_inputs(name)                                    # in addition: the host-pointer entry
    host = gpu_ctx.fcd_match(n_rows, n_cols, *(fcd._flatten(F1) + fcd._flatten(F2)), matrix=with_matrix)
    assert np.array_equal(got[0], host[0]) and np.array_equal(got[1], host[1]) and int(got[2][0]) == host[2]
    if with_matrix:
        assert np.array_equal(got[3], host[3])


def test_fcd_match_dev_does_not_allocate_and_checks_its_sizes(gpu_ctx):
    masks, n1, n2, n_rows, n_cols = dev_masks('gen_65x400_257x130')
    k = min(n1, n2)
    nws = gpu_ctx.fcd_match_workspace_bytes(n_rows, n_cols, n1, n2)
    ws, d_match, d_overlap, d_total = (chk.guarded(n, 0xFF) for n in (nws, k * 8, k * 8, 8))
    ups = [chk.upload(m) for m in masks]

    def call(ws_bytes=nws, rows=n_rows):
        gpu_ctx.fcd_match_dev(ups[0].ptr, ups[1].ptr, n1, ups[2].ptr, ups[3].ptr, n2, rows, n_cols, d_match.ptr,
                              d_overlap.ptr, d_total.ptr, ws.ptr, ws_bytes)

    chk.assert_no_allocation(call)
    assert int(d_total.numpy(np.uint64)[0]) == sim.expected('gen_65x400_257x130')['total']
    with pytest.raises(_native.PgxError, match='workspace too small'):
        call(ws_bytes=nws - 1)
    with pytest.raises(_native.PgxError, match='too large'):
        call(rows=2 ** 31)
    # no concepts: the total is zeroed on the stream, nothing else is touched
    gpu_ctx.fcd_match_dev(None, None, 0, ups[2].ptr, ups[3].ptr, n2, n_rows, n_cols, None, None, d_total.ptr, None, 0)
    assert int(d_total.numpy(np.uint64)[0]) == 0
    for g in (ws, d_match, d_overlap, d_total):
        g.assert_guards_intact()


@pytest.mark.parametrize('shape', ((5, 3), (70, 70)))
def test_lists_with_an_empty_concept(shape, gpu_ctx):
    """a concept without rows, one without columns and one without either, in both lists and in every position: their
    index arrays take no room in the upload, and they overlap nothing"""
    n_rows, n_cols = shape
    full = (tuple(range(n_rows)), tuple(range(n_cols)))
    edge = ((n_rows - 1, 0), (n_cols - 1,))
    F1 = [((), (0, 1)), full, ((1, 2), ()), edge, ((), ())]
    F2 = [edge, ((), ()), full, ((0,), ())]
    for A, B in ((F1, F2), (F2, F1), (F1[:1], F2), (F1, F2[1:2])):
        O = sim.overlaps(A, B, shape)
        want = sim.pairing(O)
        match, overlap, total = fcd.match_concept_lists(A, B, shape, ctx=gpu_ctx)
        assert np.array_equal(match, want[0]) and np.array_equal(overlap, want[1]) and total == want[2]
        assert np.array_equal(fcd.concept_overlaps(A, B, shape, ctx=gpu_ctx), O)
