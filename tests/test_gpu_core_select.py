"""Core / dominant allele selection on the device (csrc/select.hip; include/pgx.h "Core / dominant allele selection";
DESIGN.md 6i) against the numpy model of the same rules (tests/core_select_model.py, itself checked against the
reference's selections in tests/test_core_fasta_host.py), and the entry points of pangenomix_amd.core_genome /
allele_identification built on it against what the reference printed and wrote (tests/golden/core_fasta). Integer
results and bytes: every comparison is exact."""
import contextlib
import io
import itertools
import os

import numpy as np
import pytest

import allele_runs_model as runs_model
import core_select_model as model
import dev_entry_checks as dev
from pangenomix_amd import _native
from pangenomix_amd import allele_identification as ai
from pangenomix_amd import core_genome as cg
from pangenomix_amd import pangenome

pytestmark = pytest.mark.gpu

OUTPUTS = model.OUTPUTS
DTYPES = {'gene_count': np.uint32, 'best_allele': np.int32, 'best_count': np.uint32, 'mask': np.uint32, 'selected': np.int32,
          'n_selected': np.uint32}
B = 256                                # pgx_core_select_block(), asserted below: parametrize needs it at import
RUN_COUNTS = (1, 63, 64, 65, B - 1, B, B + 1, 2 * B + 1, B * B + 1)
GENOME_COUNTS = (1, 63, 64, 65, 130)
THRESHOLD_COUNTS = (1, 2, 31, 32)


def test_block_is_what_the_shapes_below_are_named_by():
    assert int(_native.lib().pgx_core_select_block()) == B


def run_dev(ctx, A, run_start, thresholds, G=None, gene_of_run=None, fill=0xFF, want=OUTPUTS, stream='null', n_genes=None):
    """core_select_dev on caller tensors (guard bands round every output and the workspace, garbage in them before the
    call) -> the dict of results; row t of 'selected' is cut at n_selected[t] AFTER checking that the rest of the row still
    holds the garbage."""
    n_alleles, n_genomes = A.shape
    n_runs, n_thr = len(run_start) - 1, len(thresholds)
    n_genes = (0 if G is None else G.shape[0]) if n_genes is None else n_genes
    sizes = {k: n_runs * 4 for k in OUTPUTS}
    sizes['selected'], sizes['n_selected'] = n_thr * n_runs * 4, n_thr * 4
    ws_bytes = _native.lib().pgx_core_select_workspace_bytes(n_alleles, n_genes, n_runs)
    assert ws_bytes > 0
    with dev.stream_scope(stream) as handle:
        d_abits = dev.upload(runs_model.pack(A))
        d_start = dev.upload(np.asarray(run_start, dtype=np.uint32))
        d_thr = dev.upload(np.asarray(thresholds, dtype=np.uint32))
        d_gbits = dev.upload(runs_model.pack(G)) if G is not None else None
        d_gene = dev.upload(np.asarray(gene_of_run, dtype=np.int32)) if gene_of_run is not None else None
        bufs = {k: dev.guarded(sizes[k], fill) for k in want}
        ws = dev.guarded(ws_bytes, fill)
        inputs = [x for x in (d_abits, d_start, d_thr, d_gbits, d_gene) if x is not None]
        with dev.unchanged(*inputs):
            ctx.core_select_dev(d_abits.ptr, n_alleles, d_gbits.ptr if d_gbits else None, n_genes, n_genomes, d_start.ptr,
                                n_runs, d_gene.ptr if d_gene else None, d_thr.ptr, n_thr,
                                *([bufs[k].ptr if k in bufs else None for k in OUTPUTS] + [ws.ptr, ws_bytes, handle]))
    out = {}
    for k, b in bufs.items():
        b.assert_guards_intact()
        out[k] = b.numpy(DTYPES[k])
    ws.assert_guards_intact()
    if 'selected' in out:
        rows = out['selected'].reshape(n_thr, n_runs)
        garbage = np.frombuffer(bytes([fill]) * 4, dtype=np.int32)[0]
        if 'n_selected' in out:
            for t in range(n_thr):
                assert (rows[t, int(out['n_selected'][t]):] == garbage).all(), 'selected was written behind n_selected'
            out['selected'] = [rows[t, :int(out['n_selected'][t])] for t in range(n_thr)]
        else:
            out['selected'] = rows
    return out


def coo(X):
    r, c = np.nonzero(X)
    return r.astype(np.int32), c.astype(np.int32)


def run_host(ctx, A, run_start, thresholds, G=None, gene_of_run=None, want=OUTPUTS, shuffle=None):
    ar, ac = coo(A)
    if shuffle is not None:
        p = shuffle.permutation(ar.size)
        ar, ac = ar[p], ac[p]
    gr, gc = coo(G) if G is not None else (None, None)
    out, dups = ctx.core_select(ar, ac, A.shape[0], A.shape[1], run_start, thresholds, gr, gc, 0 if G is None else G.shape[0],
                                gene_of_run, want=want)
    assert dups == (0, 0)
    return out


def random_case(rng, n_runs, n_genomes, n_thr, trailing=3):
    """Tables, runs of every length (empty ones included, `trailing` rows behind the last), a gene_of_run with -1 and with
    repeats, and thresholds drawn with repeats from 0, 1, n_genomes, n_genomes + 1, 2^32 - 1 and what lies between."""
    n_alleles = 2 * n_runs + 5
    A = rng.random((n_alleles, n_genomes)) < rng.random((n_alleles, 1)) * 0.8
    cuts = np.sort(rng.integers(0, n_alleles - trailing + 1, max(n_runs - 1, 0)))
    run_start = np.concatenate([[0], cuts, [n_alleles - trailing]]).astype(np.uint32)
    n_genes = max(1, n_runs // 2 + 1)
    G = rng.random((n_genes, n_genomes)) < rng.random((n_genes, 1))
    gene_of_run = rng.integers(-1, n_genes, n_runs).astype(np.int32)
    values = [0, 1, n_genomes, n_genomes + 1, 2 ** 32 - 1] + rng.integers(0, n_genomes + 2, 4).tolist()
    thresholds = rng.permutation(np.resize(rng.permutation(values), n_thr)).astype(np.uint32)
    return A, run_start, thresholds, G, gene_of_run


@pytest.mark.parametrize('n_runs', RUN_COUNTS)
def test_both_entries_equal_the_model_at_every_shape(n_runs, gpu_ctx):
    rng = np.random.default_rng(n_runs)
    genome_counts = GENOME_COUNTS if n_runs <= 2 * B + 1 else (3,)
    for k, (n_genomes, n_thr) in enumerate(itertools.product(genome_counts, THRESHOLD_COUNTS)):
        A, run_start, thresholds, G, gene_of_run = random_case(rng, n_runs, n_genomes, n_thr)
        want = model.select(A, run_start, thresholds, G, gene_of_run)
        got = run_dev(gpu_ctx, A, run_start, thresholds, G, gene_of_run, fill=dev.FILLS[k % 2],
                      stream=dev.STREAMS[(k // 2) % 2] if n_runs in (65, B + 1) else 'null')
        model.assert_equal(got, want, OUTPUTS)
        if n_thr in (2, 32):
            model.assert_equal(run_host(gpu_ctx, A, run_start, thresholds, G, gene_of_run, shuffle=rng), want, OUTPUTS)


def structures():
    rng = np.random.default_rng(5)
    A = rng.random((1203, 9)) < 0.3
    G = rng.random((4, 9)) < 0.6
    yield 'empty_runs_front_middle_end', A, [0, 0, 0, 64, 64, 100, 1203, 1203], G, [0, 1, 2, 3, 0, 1, 2]
    yield 'all_runs_empty', A, [0] * 301, G, [i % 4 for i in range(300)]
    yield 'one_run_holds_1000_alleles', A, [0, 100, 1100, 1203], G, [3, 2, 1]
    yield 'rows_behind_the_last_run', A, [0, 10, 64, 150], G, [0, 1, 2]
    yield 'no_gene_row_and_two_runs_on_one_gene', A, [0, 300, 600, 900, 1203], G, [2, -1, 2, -1]
    yield 'single_rows', A[:600], list(range(601)), G, [i % 5 - 1 for i in range(600)]
    Z = A.copy()
    Z[100:1100] = False                                     # a run whose rows are all empty still has a first row
    yield 'rows_without_entries', Z, [0, 100, 1100, 1203], G, [0, 1, 2]


STRUCTURES = list(structures())
# what the Python layer asks for, then every other combination that takes another path through the entry
WANTS = (('gene_count', 'selected', 'n_selected'), ('gene_count',), ('mask',), ('best_allele', 'best_count'), ('n_selected',),
         ('selected',), ('best_count', 'mask', 'selected', 'n_selected'))


@pytest.mark.parametrize('name,A,run_start,G,gene_of_run', STRUCTURES, ids=[x[0] for x in STRUCTURES])
def test_run_structures_and_null_outputs(name, A, run_start, G, gene_of_run, gpu_ctx):
    thresholds = [5, 0, 2 ** 32 - 1, 9, 5, 10, 1]
    want = model.select(A, run_start, thresholds, G, gene_of_run)
    model.assert_equal(run_dev(gpu_ctx, A, run_start, thresholds, G, gene_of_run, stream='side'), want, OUTPUTS)
    model.assert_equal(run_host(gpu_ctx, A, run_start, thresholds, G, gene_of_run), want, OUTPUTS)
    for k, keys in enumerate(WANTS):
        got = run_dev(gpu_ctx, A, run_start, thresholds, G, gene_of_run, want=keys, fill=dev.FILLS[k % 2])
        assert sorted(got) == sorted(keys)
        if 'n_selected' not in keys and 'selected' in keys:     # rows not cut: compare what the model says was written
            rows = got.pop('selected')
            for t, sel in enumerate(want['selected']):
                assert np.array_equal(rows[t, :sel.size], sel)
        model.assert_equal(got, want)
    host = run_host(gpu_ctx, A, run_start, thresholds, G, gene_of_run, want=WANTS[0])
    assert sorted(host) == sorted(WANTS[0])
    model.assert_equal(host, want)
    # no gene_of_run: every non-empty run is eligible, every gene count is 0
    free = model.select(A, run_start, thresholds)
    model.assert_equal(run_dev(gpu_ctx, A, run_start, thresholds), free, OUTPUTS)
    model.assert_equal(run_host(gpu_ctx, A, run_start, thresholds), free, OUTPUTS)
    # gene_of_run without a gene bitmap (the device entry only): eligible by gene_of_run, every gene count 0
    bare = model.select(A, run_start, thresholds, None, gene_of_run)
    model.assert_equal(run_dev(gpu_ctx, A, run_start, thresholds, None, gene_of_run, n_genes=G.shape[0]), bare, OUTPUTS)


def test_two_calls_return_equal_bytes_and_allocate_nothing(gpu_ctx):
    rng = np.random.default_rng(8)
    A, run_start, thresholds, G, gene_of_run = random_case(rng, 3 * B + 7, 65, 32)
    results = []
    for fill in dev.FILLS + dev.FILLS[:1]:
        got = run_dev(gpu_ctx, A, run_start, thresholds, G, gene_of_run, fill=fill)
        results.append(tuple(got[k] for k in OUTPUTS if k != 'selected') + tuple(got['selected']))
    dev.same_bytes(results)
    host = [run_host(gpu_ctx, A, run_start, thresholds, G, gene_of_run) for _ in range(2)]
    dev.same_bytes([tuple(h[k] for k in OUTPUTS if k != 'selected') + tuple(h['selected']) for h in host])
    n_alleles, n_genomes = A.shape
    n_runs = len(run_start) - 1
    ws_bytes = _native.lib().pgx_core_select_workspace_bytes(n_alleles, G.shape[0], n_runs)
    d = [dev.upload(x) for x in (runs_model.pack(A), runs_model.pack(G), run_start, gene_of_run, thresholds)]
    outs = [dev.guarded(n_runs * 4 * (32 if k == 'selected' else 1) if k != 'n_selected' else 128, 0xFF) for k in OUTPUTS]
    ws = dev.guarded(ws_bytes, 0xFF)
    dev.assert_no_allocation(lambda: gpu_ctx.core_select_dev(d[0].ptr, n_alleles, d[1].ptr, G.shape[0], n_genomes, d[2].ptr, n_runs,
                                                             d[3].ptr, d[4].ptr, 32, *([o.ptr for o in outs] + [ws.ptr, ws_bytes])))


def test_dev_entry_refuses_bad_arguments_without_a_fault(gpu_ctx):
    A = np.ones((100, 3), dtype=bool)
    G = np.ones((2, 3), dtype=bool)
    for run_start, gene_of_run, match in (([0, 50, 40, 100], [0, 0, 0], 'never decrease'), ([0, 50, 101], [0, 1], 'beyond'),
                                          ([1, 50, 100], [0, 1], 'start at 0'), ([0, 50, 100], [0, 2], 'gene_of_run'),
                                          ([0, 50, 100], [0, -2], 'gene_of_run'),
                                          ([0, 2 ** 31, 2 ** 32 - 1], [2 ** 31 - 1, -2 ** 31], 'beyond')):
        with pytest.raises(_native.PgxError, match=match) as e:
            run_dev(gpu_ctx, A, run_start, [1, 2], G, gene_of_run)          # (guards and inputs are checked on the way)
        assert e.value.status == -1
    d = dev.upload(runs_model.pack(A))
    s = dev.upload(np.array([0, 100], dtype=np.uint32))
    t = dev.upload(np.arange(40, dtype=np.uint32))
    out = dev.guarded(4, 0xFF)
    ws_bytes = _native.lib().pgx_core_select_workspace_bytes(100, 0, 1)
    ws = dev.guarded(ws_bytes, 0xFF)

    def call(n_runs=1, thresholds=t.ptr, n_thr=1, result=out.ptr, workspace=ws.ptr, size=ws_bytes):
        gpu_ctx.core_select_dev(d.ptr, 100, None, 0, 3, s.ptr, n_runs, None, thresholds, n_thr, None, result, None, None, None,
                                None, workspace, size)

    for kwargs, match in ((dict(n_thr=0), '1..32'), (dict(n_thr=33), '1..32'), (dict(thresholds=None), 'NULL thresholds'),
                          (dict(size=ws_bytes - 256), 'workspace too small'), (dict(workspace=None, size=0), 'workspace too small'),
                          (dict(workspace=ws.ptr + 4), '16-byte aligned'), (dict(n_runs=0), 'no runs')):
        with pytest.raises(_native.PgxError, match=match) as e:
            call(**kwargs)
        assert e.value.status == -1
    assert out.is_still_garbage() and ws.is_still_garbage()
    call(n_runs=0, result=None, workspace=None, size=0)                     # no runs and nothing asked for: fine
    assert _native.lib().pgx_core_select_workspace_bytes(2 ** 31, 1, 1) == 0
    call()
    assert out.numpy(np.int32)[0] == 0
    out.assert_guards_intact()


def test_host_entry_reports_duplicates_and_refuses_before_any_launch(gpu_ctx):
    A = np.ones((10, 3), dtype=bool)
    G = np.ones((2, 3), dtype=bool)
    (ar, ac), (gr, gc) = coo(A), coo(G)
    ok = dict(n_alleles=10, n_genomes=3, run_start=[0, 5, 10], thresholds=[1, 3], gene_rows=gr, gene_genomes=gc, n_genes=2,
              gene_of_run=[0, 1])
    out, dups = gpu_ctx.core_select(np.append(ar, ar[:2]), np.append(ac, ac[:2]), **ok)
    assert out is None and dups == (2, 0)
    out, dups = gpu_ctx.core_select(ar, ac, **dict(ok, gene_rows=np.append(gr, gr[:1]), gene_genomes=np.append(gc, gc[:1])))
    assert out is None and dups == (0, 1)
    gpu_ctx.profile(True)
    gpu_ctx.profile_reset()
    try:
        for change, match in ((dict(run_start=[0, 6, 5, 10], gene_of_run=[0, 1, 1]), 'never decrease'),
                              (dict(run_start=[0, 5, 11]), 'beyond'), (dict(gene_of_run=[0, 2]), 'gene_of_run'),
                              (dict(run_start=[0], gene_of_run=[]), 'no runs'), (dict(run_start=[2, 5, 10]), 'start at 0'),
                              (dict(thresholds=[]), '1..32'), (dict(thresholds=list(range(33))), '1..32')):
            with pytest.raises(_native.PgxError, match=match) as e:
                gpu_ctx.core_select(ar, ac, **dict(ok, **change))
            assert e.value.status == -1
        assert sum(n for _, n in gpu_ctx.profile_read().values()) == 0     # nothing was launched
    finally:
        gpu_ctx.profile(False)
    with pytest.raises(_native.PgxError, match='out of range'):
        gpu_ctx.core_select(np.array([10]), np.array([0]), **ok)
    out, dups = gpu_ctx.core_select(ar, ac, 10, 3, [0], [1], want=())       # no runs and nothing asked for: fine
    assert out == {} and dups == (0, 0)
    out, dups = gpu_ctx.core_select(ar, ac, **ok)
    assert out['selected'][0].tolist() == [0, 5] and out['n_selected'].tolist() == [2, 2] and out['mask'].tolist() == [3, 3]


# -- the entry points of the Python layer ------------------------------------------------------------------------------
def captured(fn, *args, **kwargs):
    buf = io.StringIO()
    value = error = None
    with contextlib.redirect_stdout(buf):
        try:
            value = fn(*args, **kwargs)
        except (KeyError, ValueError) as e:
            error = e
    return value, error, buf.getvalue()


@pytest.mark.parametrize('case', sorted(model.CORE_CASES))
def test_create_core_genes_fasta_writes_and_prints_what_the_reference_did(case, gpu_ctx, tmp_path):
    inputs, genomes_num = model.CORE_CASES[case]
    f, want = model.INPUTS[inputs], model.load_case(case)
    out = str(tmp_path / 'out.faa')
    _, error, text = captured(cg.create_core_genes_fasta, f['allele_npz'], f['allele_labels'], f['gene_npz'], f['gene_labels'],
                              f['faa'], genomes_num, out, ctx=gpu_ctx)
    assert text == want['stdout']
    if want['raises_whole']:
        assert type(error).__name__ == want['raises_whole']['type'] and [str(a) for a in error.args] == want['raises_whole']['args']
        assert not os.path.exists(out)
    else:
        assert error is None and open(out, 'rb').read() == want['out_faa']


def test_create_core_genes_fasta_serves_many_thresholds_in_one_call(gpu_ctx, tmp_path):
    for inputs, nums, cases in (('hand', [5, 3, 1, 2.5, 3], ('hand_core_5', 'hand_core_3', 'hand_core_1', 'hand_core_3', 'hand_core_3')),
                                ('cds', (3, 1), ('cds_core_3', 'cds_core_1'))):
        f = model.INPUTS[inputs]
        outs = [str(tmp_path / ('%s_%d.faa' % (inputs, i))) for i in range(len(nums))]
        gpu_ctx.profile(True)
        gpu_ctx.profile_reset()
        try:
            _, error, text = captured(cg.create_core_genes_fasta, f['allele_npz'], f['allele_labels'], f['gene_npz'],
                                      f['gene_labels'], f['faa'], nums, outs, ctx=gpu_ctx)
            launches = {name: n for name, (_, n) in gpu_ctx.profile_read().items()}
        finally:
            gpu_ctx.profile(False)
        assert error is None
        assert launches['select_mask_kernel'] == launches['select_scan_kernel'] == launches['select_scatter_kernel'] == 1
        one = model.load_case(cases[0])['stdout']
        assert text == one[:one.index('\nFound')] + one[one.index('\nFound'):] * len(nums)
        for path, case in zip(outs, cases):
            assert open(path, 'rb').read() == model.load_case(case)['out_faa']
    outs = [str(tmp_path / ('none%d.faa' % i)) for i in range(2)]
    _, error, _ = captured(cg.create_core_genes_fasta, f['allele_npz'], f['allele_labels'], f['gene_npz'], f['gene_labels'],
                           f['faa'], (1, 7), outs, ctx=gpu_ctx)
    assert isinstance(error, KeyError) and error.args == ('gene_index',) and not any(os.path.exists(p) for p in outs)


@pytest.mark.parametrize('case', sorted(model.ALLELE_CASES))
def test_create_alleles_fasta_writes_and_prints_what_the_reference_did(case, gpu_ctx, tmp_path):
    f, want = model.INPUTS[model.ALLELE_CASES[case]], model.load_case(case)
    out = str(tmp_path / 'out.faa')
    _, error, text = captured(ai.create_alleles_fasta, f['allele_npz'], f['gene_labels'], f['allele_labels'], f['faa'], out,
                              ctx=gpu_ctx)
    assert error is None and text == want['stdout']
    assert open(out, 'rb').read() == want['out_faa']


def test_core_allele_sets_equals_the_helpers_chained_by_hand(gpu_ctx):
    for inputs, nums in (('cds', [1, 3, 7, 2.0, 6]), ('hand', [6, 5, 4, 3, 2, 1])):
        f = model.INPUTS[inputs]
        got, error, text = captured(cg.core_allele_sets, f['allele_npz'], f['allele_labels'], f['gene_npz'], f['gene_labels'],
                                    nums, ctx=gpu_ctx)
        assert error is None and text == ''
        with contextlib.redirect_stdout(io.StringIO()):
            alleles = cg.count_allele_occurence(f['allele_npz'], ctx=gpu_ctx)
            genes = cg.count_gene_occurence(f['gene_npz'], ctx=gpu_ctx)
            pairs = cg.identify_gene_allele_rows(f['gene_labels'], f['allele_labels'])
            for k, names in zip(nums, got):
                core = cg.find_core_genes(genes, k)
                if core.empty:
                    assert names.size == 0
                    continue
                rows = cg.find_highest_allele_expression(alleles, cg.subset_genes_alleles_pairs(pairs, core))
                assert names.tolist() == cg.find_allele_names(rows, f['allele_labels']).tolist()


def test_both_workflows_on_the_files_build_cds_pangenome_wrote(gpu_ctx, tmp_path, golden_dir):
    src = os.path.join(golden_dir, 'cds', 'in')
    paths = sorted(os.path.join(src, f) for f in os.listdir(src) if f.endswith('.faa'))
    out_dir = tmp_path / 'out'
    out_dir.mkdir()
    with contextlib.redirect_stdout(io.StringIO()):
        pangenome.build_cds_pangenome(paths, str(out_dir), name='T')
    a_npz, g_npz = str(out_dir / 'T_strain_by_allele.npz'), str(out_dir / 'T_strain_by_gene.npz')
    files = {'allele_npz': a_npz, 'allele_labels': a_npz + '.labels.txt', 'gene_npz': g_npz, 'gene_labels': g_npz + '.labels.txt',
             'faa': str(out_dir / 'T_nr.faa')}
    got, want = str(tmp_path / 'got.faa'), str(tmp_path / 'want.faa')
    # (the clusters are the device's own, so the tables are not those of the fixtures: the model selects on the files
    # written, and filter_sequences -- host code, checked against the fixtures -- writes what is expected)
    for k in (1, 3):
        names = model.reference_selection(files, [k])[0]
        assert names
        _, error, _ = captured(cg.create_core_genes_fasta, files['allele_npz'], files['allele_labels'], files['gene_npz'],
                               files['gene_labels'], files['faa'], k, got, ctx=gpu_ctx)
        captured(cg.filter_sequences, files['faa'], names, want)
        assert error is None and open(got, 'rb').read() == open(want, 'rb').read() != b''
    names = model.reference_selection(files, [0], with_gene_table=False)[0]
    _, error, _ = captured(ai.create_alleles_fasta, files['allele_npz'], files['gene_labels'], files['allele_labels'], files['faa'],
                           got, ctx=gpu_ctx)
    captured(cg.filter_sequences, files['faa'], names, want)
    assert error is None and open(got, 'rb').read() == open(want, 'rb').read() != b''
    assert open(got, 'rb').read().count(b'>') == len(names)


# -- the host entry's transfers ----------------------------------------------------------------------------------------
def small_case(n_genomes):
    """Five runs (one empty, one without a gene row) and thresholds that select none, some and all of the eligible runs."""
    rng = np.random.default_rng(n_genomes)
    A = rng.random((12, n_genomes)) < 0.5
    A[0] = True
    run_start = np.array([0, 2, 2, 5, 9, 12], dtype=np.uint32)
    G = np.zeros((3, n_genomes), dtype=bool)
    G[0], G[1, :2], G[2, :1] = True, True, True
    gene_of_run = np.array([0, 1, 1, -1, 2], dtype=np.int32)
    thresholds = np.array([2 ** 32 - 1, 2, 0, n_genomes], dtype=np.uint32)
    return A, run_start, thresholds, G, gene_of_run


@pytest.mark.parametrize('n_genomes', (3, 70))
def test_host_entry_with_rows_of_selected_that_are_empty_short_and_alone(n_genomes, gpu_ctx):
    A, run_start, thresholds, G, gene_of_run = small_case(n_genomes)
    n_runs = run_start.size - 1
    want = model.select(A, run_start, thresholds, G, gene_of_run)
    sizes = [s.size for s in want['selected']]
    assert sizes[0] == 0 and 0 < sizes[1] < sizes[2] < n_runs and sizes[3] == 1
    model.assert_equal(run_host(gpu_ctx, A, run_start, thresholds, G, gene_of_run), want, OUTPUTS)
    for keys in (('mask',), ('selected',), ('n_selected',), ('gene_count',)):
        got = run_host(gpu_ctx, A, run_start, thresholds, G, gene_of_run, want=keys)
        assert set(keys) <= set(got) <= set(keys) | {'n_selected'}
        model.assert_equal(got, want)
    free = model.select(A, run_start, thresholds)                            # no gene table
    for keys in (OUTPUTS, ('mask',), ('selected',)):
        model.assert_equal(run_host(gpu_ctx, A, run_start, thresholds, want=keys), free)


def test_host_entry_leaves_selected_behind_n_selected_as_the_caller_had_it(gpu_ctx):
    lib, P, h = _native.lib(), _native._ptr, gpu_ctx._h
    A, run_start, thresholds, G, gene_of_run = small_case(3)
    n_runs, n_thr = run_start.size - 1, thresholds.size
    want = model.select(A, run_start, thresholds, G, gene_of_run)
    (ar, ac), (gr, gc) = coo(A), coo(G)
    sentinel = 0x5C5C5C5C
    selected = np.full((n_thr, n_runs), sentinel, dtype=np.int32)
    n_selected = np.full(n_thr, sentinel, dtype=np.uint32)
    dup = np.zeros(2, dtype=np.uint64)
    rc = lib.pgx_core_select(h, P(ar), P(ac), ar.size, A.shape[0], P(gr), P(gc), gr.size, G.shape[0], A.shape[1], P(run_start),
                             n_runs, P(gene_of_run), P(thresholds), n_thr, None, None, None, None, P(selected), P(n_selected),
                             P(dup))
    assert rc == 0 and dup.tolist() == [0, 0]
    assert n_selected.tolist() == [s.size for s in want['selected']]
    for t, sel in enumerate(want['selected']):
        assert selected[t, :sel.size].tolist() == sel.tolist()
        assert (selected[t, sel.size:] == sentinel).all(), 'row %d was written behind n_selected' % t
