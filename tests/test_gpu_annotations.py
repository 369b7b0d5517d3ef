"""The device step of extract_annotations (csrc/annot.hip; include/pgx.h "Ordered de-duplication of rows of ids and the
plurality vote of runs of rows") against the plain-Python model of tests/annot_model.py, and the ctx= layer of
pangenomix_amd.pangenome on a real context against what the reference wrote (tests/golden/annotations) and against the host
path. Integers and bytes: every comparison is exact. Every set runs twice, the second time with PGX_ANNOT_NARROW_HASH: 3 bits
of hash, every probe collides, same output."""
import numpy as np
import pytest

import annot_model as model
import annotations_cases as cases
import dev_entry_checks as dev
from pangenomix_amd import _native, pangenome as pg

pytestmark = pytest.mark.gpu

NARROW = 1                                   # PGX_ANNOT_NARROW_HASH
FLAGS = (0, NARROW)


def row_tile():
    return int(_native.lib().pgx_annot_row_tile())


def run_tile():
    return int(_native.lib().pgx_annot_run_tile())


def check_vote(ctx, rows, run_off, flags, want=None):
    want = want or model.vote_fast(rows, run_off)
    tok, row_off = model.flatten(rows)
    got = ctx.annot_vote(tok, row_off, run_off, flags)
    again = ctx.annot_vote(tok, row_off, run_off, flags)
    for name, g, a, w in zip(('keep', 'winner', 'votes', 'differs'), got, again, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert np.array_equal(g, w), '%s differs first at %d' % (name, int(np.flatnonzero(g != w)[0]))
        assert g.tobytes() == a.tobytes(), '%s differs between two calls' % name
    return got


def singles(rows):
    return np.arange(len(rows) + 1, dtype=np.uint32)


# -- rows --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('flags', FLAGS)
def test_row_lengths_around_the_lane_group_and_the_long_row_path(flags, gpu_ctx):
    T = row_tile()
    assert T >= 16
    rng = np.random.default_rng(11)
    rows = []
    for length in sorted({0, 1, 2, 15, 16, 17, 63, 64, 65, T - 1, T, T + 1, 4 * T}):
        rows += model.row_shapes(length, rng)
    keep, winner, votes, differs = check_vote(gpu_ctx, rows, singles(rows), flags)
    assert (votes == 1).all() and not differs.any() and winner.tolist() == list(range(len(rows)))
    # the same rows as runs of equal pairs: a row of repeats equals the row it collapses to
    pairs = [r for row in rows for r in (row, list(row))]
    keep, winner, votes, differs = check_vote(gpu_ctx, pairs, np.arange(0, len(pairs) + 1, 2, dtype=np.uint32), flags)
    assert (votes == 2).all() and not differs.any()


@pytest.mark.parametrize('flags', FLAGS)
def test_a_long_row_with_more_distinct_ids_than_its_set_takes_at_once(flags, gpu_ctx):
    """3000 distinct ids, every one a second time further on, and a tail of repeats: several rounds of the long-row path"""
    rng = np.random.default_rng(12)
    ids = [int(x) for x in rng.permutation(1 << 20)[:3000]]
    row = ids + [int(x) for x in rng.permutation(ids)] + ids[-40:]
    rows = [row, ids, list(reversed(ids)), row[:3000 + 5]]
    keep, winner, votes, differs = check_vote(gpu_ctx, rows, np.array([0, 4], dtype=np.uint32), flags)
    assert int(keep[:len(row)].sum()) == 3000 and winner.tolist() == [0] and votes.tolist() == [3]
    assert differs.tolist() == [0, 0, 1, 0]


# -- runs --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('flags', FLAGS)
def test_run_sizes_around_the_wave_and_the_workgroup_path(flags, gpu_ctx):
    U = run_tile()
    rng = np.random.default_rng(13)
    rows, run_off = [], [0]
    for size in sorted({1, 2, 63, 64, 65, U - 1, U, U + 1}):
        for kind in ('equal', 'distinct', 'tie', 'mixed'):
            rows += model.run_of(size, kind, rng)
            run_off.append(len(rows))
    run_off = np.array(run_off, dtype=np.uint32)
    want = model.vote(rows, run_off)                        # the definition itself, where its quadratic count is affordable
    assert all(np.array_equal(a, b) for a, b in zip(want, model.vote_fast(rows, run_off)))
    check_vote(gpu_ctx, rows, run_off, flags, want)


@pytest.mark.parametrize('flags', FLAGS)
@pytest.mark.parametrize('kind', ('equal', 'distinct', 'tie', 'mixed'))
def test_a_run_of_5000_rows_between_short_ones(kind, flags, gpu_ctx):
    rng = np.random.default_rng(14)
    before, big, after = model.run_of(3, 'mixed', rng), model.run_of(5000, kind, rng), model.run_of(2, 'tie', rng)
    rows = before + big + after
    run_off = np.array([0, 3, 5003, 5005], dtype=np.uint32)
    keep, winner, votes, differs = check_vote(gpu_ctx, rows, run_off, flags)
    if kind == 'equal':
        assert votes[1] == 5000 and winner[1] == 3
    if kind == 'distinct':
        assert votes[1] == 1 and winner[1] == 3 and differs[3:5003].sum() == 4999
    if kind == 'tie':
        assert votes[1] == 2500 and winner[1] == 3 and rows[3] == [8, 4]


@pytest.mark.parametrize('flags', FLAGS)
def test_lists_that_are_nearly_equal(flags, gpu_ctx):
    """a prefix of another, the same set in another order, [a, b] against [a, a, b], empty rows"""
    a, b, c = 3, 70000, (1 << 31) - 1
    rows = [[a, b], [a, b, c], [b, a], [a, a, b], [a], [], [], [a, b, a, b], [c], [a, b, c, c]]
    for run_off in ([0, 10], [0, 4, 7, 10], list(range(11))):
        keep, winner, votes, differs = check_vote(gpu_ctx, rows, np.array(run_off, dtype=np.uint32), flags, model.vote(rows, run_off))
    keep, winner, votes, differs = check_vote(gpu_ctx, rows, np.array([0, 10], dtype=np.uint32), flags)
    assert winner.tolist() == [0] and votes.tolist() == [3] and differs.tolist() == [0, 1, 1, 0, 1, 1, 1, 0, 1, 1]
    # and the same lists spread over a long run
    rng = np.random.default_rng(15)
    many = [list(rows[int(i)]) for i in rng.integers(0, len(rows), 700)]
    check_vote(gpu_ctx, many, np.array([0, 700], dtype=np.uint32), flags)


@pytest.mark.parametrize('flags', FLAGS)
def test_many_short_rows_and_runs_like_a_names_file(flags, gpu_ctx):
    rng = np.random.default_rng(16)
    rows = [[int(x) for x in rng.integers(0, 40, int(k))] for k in rng.integers(0, 4, 6000)]
    sizes = rng.integers(1, 5, 4000)
    run_off = np.concatenate(([0], np.cumsum(sizes)))
    run_off = run_off[run_off < len(rows)].tolist() + [len(rows)]
    check_vote(gpu_ctx, rows, np.array(run_off, dtype=np.uint32), flags)


def test_no_rows(gpu_ctx):
    got = gpu_ctx.annot_vote(np.zeros(0, dtype=np.int32), np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint32))
    assert [g.size for g in got] == [0, 0, 0, 0]
    gpu_ctx.annot_vote_dev(None, None, 0, 0, None, 0, None, None, None, None, None, 0)


# -- the device-pointer entry ------------------------------------------------------------------------------------------------
def dev_case(seed):
    rng = np.random.default_rng(seed)
    rows = []
    run_off = [0]
    for size, kind in ((3, 'mixed'), (run_tile() + 6, 'mixed'), (1, 'equal'), (300, 'tie'), (run_tile(), 'mixed')):
        rows += model.run_of(size, kind, rng)
        run_off.append(len(rows))
    rows[1] = [int(x) for x in rng.integers(0, 50, row_tile() + 9)]
    rows[5] = [int(x) for x in rng.integers(0, 5000, 3 * row_tile())]
    return rows, np.array(run_off, dtype=np.uint32)


def run_vote_dev(ctx, rows, run_off, flags, fill, stream):
    want = model.vote_fast(rows, run_off)
    tok, row_off = model.flatten(rows)
    n_rows, n_tokens, n_runs = len(rows), int(tok.size), int(run_off.size - 1)
    ws_bytes = ctx.annot_vote_workspace_bytes(n_rows, n_tokens, n_runs)
    assert ws_bytes > 0
    with dev.stream_scope(stream) as handle:
        d_tok, d_row, d_run = dev.upload(tok), dev.upload(row_off), dev.upload(run_off)
        keep, winner, votes, differs, ws = (dev.guarded(n_tokens, fill), dev.guarded(4 * n_runs, fill),
                                            dev.guarded(4 * n_runs, fill), dev.guarded(n_rows, fill),
                                            dev.guarded(ws_bytes, fill))
        with dev.unchanged(d_tok, d_row, d_run):
            ctx.annot_vote_dev(d_tok.ptr, d_row.ptr, n_rows, n_tokens, d_run.ptr, n_runs, keep.ptr, winner.ptr, votes.ptr,
                               differs.ptr, ws.ptr, ws_bytes, flags, handle)
    for buf in (keep, winner, votes, differs, ws):
        buf.assert_guards_intact()
    got = keep.numpy(np.uint8), winner.numpy(np.int32), votes.numpy(np.uint32), differs.numpy(np.uint8)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    return got


@pytest.mark.parametrize('flags', FLAGS)
@pytest.mark.parametrize('stream', dev.STREAMS)
def test_vote_device_entry_on_caller_tensors(stream, flags, gpu_ctx):
    for seed in (1, 2):
        case = dev_case(seed)
        dev.same_bytes([run_vote_dev(gpu_ctx, *case, flags, fill, stream) for fill in dev.FILLS])


def test_vote_device_entry_does_not_allocate(gpu_ctx):
    rows, run_off = dev_case(3)
    tok, row_off = model.flatten(rows)
    n_rows, n_tokens, n_runs = len(rows), int(tok.size), int(run_off.size - 1)
    ws_bytes = gpu_ctx.annot_vote_workspace_bytes(n_rows, n_tokens, n_runs)
    d_tok, d_row, d_run = dev.upload(tok), dev.upload(row_off), dev.upload(run_off)
    keep, winner, votes, differs, ws = (dev.guarded(n_tokens, 0xFF), dev.guarded(4 * n_runs, 0xFF), dev.guarded(4 * n_runs, 0xFF),
                                        dev.guarded(n_rows, 0xFF), dev.guarded(ws_bytes, 0xFF))
    dev.assert_no_allocation(lambda: gpu_ctx.annot_vote_dev(d_tok.ptr, d_row.ptr, n_rows, n_tokens, d_run.ptr, n_runs, keep.ptr,
                                                            winner.ptr, votes.ptr, differs.ptr, ws.ptr, ws_bytes))
    assert np.array_equal(winner.numpy(np.int32), model.vote_fast(rows, run_off)[1])


def test_invalid_calls_are_refused_before_anything_is_written(gpu_ctx):
    lib, P, h = _native.lib(), _native._ptr, gpu_ctx._h
    tok = np.array([1, 2, 2, 3, 1], dtype=np.int32)
    row_off, run_off = np.array([0, 2, 3, 5], dtype=np.uint64), np.array([0, 2, 3], dtype=np.uint32)
    keep, differs = np.full(5, 0x6E, dtype=np.uint8), np.full(3, 0x6E, dtype=np.uint8)
    winner, votes = np.full(2, 0x6E6E6E6E, dtype=np.int32), np.full(2, 0x6E6E6E6E, dtype=np.uint32)

    def call(t=tok, ro=row_off, n_rows=3, ru=run_off, n_runs=2, flags=0):
        return lib.pgx_annot_vote(h, P(t), P(ro), n_rows, P(ru), n_runs, flags, P(keep), P(winner), P(votes), P(differs))

    def refused(rc, who):
        assert rc == -1, who                                # PGX_ERR_INVALID
        assert (keep == 0x6E).all() and (differs == 0x6E).all() and (winner == 0x6E6E6E6E).all(), who
        assert (votes == 0x6E6E6E6E).all(), who
    refused(call(flags=2), 'flags')
    refused(call(ro=np.array([0, 3, 2, 5], dtype=np.uint64)), 'decreasing offsets')
    refused(call(ro=np.array([1, 2, 3, 5], dtype=np.uint64)), 'offsets that do not start at 0')
    refused(call(ro=np.array([0, 2, 3, 1 << 31], dtype=np.uint64)), '2^31 tokens')
    refused(call(ru=np.array([0, 2, 2], dtype=np.uint32)), 'an empty run')
    refused(call(ru=np.array([0, 2, 4], dtype=np.uint32)), 'a run past the rows')
    refused(call(ru=np.array([0, 1, 2], dtype=np.uint32)), 'runs that leave a row out')
    refused(call(ru=np.array([1, 2, 3], dtype=np.uint32)), 'runs that do not start at 0')
    refused(call(ru=np.array([0, 3, 2], dtype=np.uint32)), 'decreasing runs')
    refused(call(n_runs=0), 'rows without a run')
    refused(call(t=np.array([1, 2, -1, 3, 1], dtype=np.int32)), 'a negative id')
    big = np.zeros((1 << 24) + 1, dtype=np.uint64)
    refused(call(ro=big, n_rows=1 << 24), 'n_rows')
    assert lib.pgx_annot_vote_workspace_bytes(1 << 24, 0, 1) == 0 and lib.pgx_annot_vote_workspace_bytes(3, 1 << 31, 1) == 0
    assert call() == 0
    assert keep.tolist() == [1, 1, 1, 1, 1] and winner.tolist() == [0, 2] and votes.tolist() == [1, 1]
    assert differs.tolist() == [0, 1, 0]
    # the device entry refuses the same without touching its buffers
    g = dev.guarded(4096, 0x5A)
    ws_bytes = gpu_ctx.annot_vote_workspace_bytes(3, 5, 2)
    for n_rows, n_tokens, n_runs, flags, ws in ((1 << 24, 5, 2, 0, 1 << 30), (3, 1 << 31, 2, 0, 1 << 30), (3, 5, 2, 2, ws_bytes),
                                                (3, 5, 2, 0, ws_bytes - 8), (3, 5, 2, 0, 0), (3, 5, 4, 0, ws_bytes),
                                                (3, 5, 0, 0, ws_bytes)):
        with pytest.raises(_native.PgxError) as e:
            gpu_ctx.annot_vote_dev(g.ptr, g.ptr, n_rows, n_tokens, g.ptr, n_runs, g.ptr, g.ptr, g.ptr, g.ptr, g.ptr, ws, flags)
        assert e.value.status == -1
    assert g.is_still_garbage()
    g.assert_guards_intact()


# -- the Python layer on a real context --------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', cases.EXTRACT_CASES)
def test_extract_annotations_equals_the_reference_and_the_host_path(case, gpu_ctx, tmp_path, capsys):
    """file bytes, stdout, the exception, no .tmp left -- and the path that ran: the device for every regular case, the
    host for every irregular one"""
    want = cases.run_extract(case, tmp_path / 'host', capsys, ctx=None)
    cases.assert_recorded(case, want)
    pg.ANNOTATION_PATH_COUNTS.clear()
    got = cases.run_extract(case, tmp_path / 'device', capsys, ctx=gpu_ctx)
    assert got == want
    regular = cases.load_case(case)['regular']
    assert dict(pg.ANNOTATION_PATH_COUNTS) == ({'extract_device': 1} if regular else {'extract_host': 1})


@pytest.mark.parametrize('case', cases.GENERATE_CASES)
def test_generate_annotations_equals_the_reference_and_the_host_path(case, gpu_ctx, tmp_path):
    want = cases.run_generate(case, tmp_path, ctx=None)
    cases.assert_recorded(case, want)
    pg.ANNOTATION_PATH_COUNTS.clear()
    got = cases.run_generate(case, tmp_path, ctx=gpu_ctx)
    assert got == want
    raises = want['exception'] is not None
    assert dict(pg.ANNOTATION_PATH_COUNTS) == ({'generate_host': 1} if raises else {'generate_device': 1})


def test_extract_annotations_on_a_generated_names_file(gpu_ctx, tmp_path, capsys):
    """a few hundred genes with runs and rows on both sides of the tiles, percent-encoded products, both batch sizes"""
    gffs, names = cases.generated_set(tmp_path, n_genomes=5, n_genes=300, big_run=run_tile() + 40, big_row=row_tile() + 30)
    for kw in (dict(batch=100), dict(batch=2), dict(collapse_alleles=False), dict(flexible_locus_tag=True)):
        out_h, out_d = str(tmp_path / 'h.tsv'), str(tmp_path / 'd.tsv')
        pg.extract_annotations(gffs, names, out_h, **kw)
        printed_h = capsys.readouterr().out
        pg.ANNOTATION_PATH_COUNTS.clear()
        pg.extract_annotations(gffs, names, out_d, ctx=gpu_ctx, **kw)
        assert capsys.readouterr().out == printed_h
        assert dict(pg.ANNOTATION_PATH_COUNTS) == {'extract_device': 1}
        assert open(out_d, 'rb').read() == open(out_h, 'rb').read() and len(open(out_h, 'rb').read()) > 1000


@pytest.mark.parametrize('flags', FLAGS)
@pytest.mark.parametrize('n_rows', (3, 70))
def test_rows_that_are_all_empty(n_rows, flags, gpu_ctx):
    """no id at all: nothing goes up but the offsets, `keep` has no entry, and every run's winner is its first row"""
    rows = [[] for _ in range(n_rows)]
    for run_off in ([0, n_rows], [0, 1, n_rows], list(range(n_rows + 1))):
        run_off = np.array(run_off, dtype=np.uint32)
        keep, winner, votes, differs = check_vote(gpu_ctx, rows, run_off, flags, model.vote(rows, run_off))
        assert keep.size == 0 and winner.tolist() == run_off[:-1].tolist() and not differs.any()
        assert votes.tolist() == np.diff(run_off).tolist()
