"""Runs of allele rows on the device (csrc/runs.hip; include/pgx.h "Runs of allele rows") against the numpy
model of the same rules (tests/allele_runs_model.py, itself checked against the reference's recorded output in
tests/test_consistency_host.py), and the three functions of pangenomix_amd.pangenome built on them against what the
reference printed, returned and wrote (tests/golden/consistency). Integer results: every comparison is exact."""
import contextlib
import glob
import io
import os

import numpy as np
import pytest
import scipy.sparse

import allele_runs_model as model
import dev_entry_checks as dev
from pangenomix_amd import _native, pangenome, sparse_utils

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted(glob.glob(os.path.join(model.GOLDEN, '*.npz')))
ids = [os.path.basename(p)[:-4] for p in CASES]
OUTPUTS = _native.Context.RUNS_OUTPUTS
DTYPES = {'derived': np.uint64, 'diff': np.uint64, 'diff_per_genome': np.uint32, 'diff_per_run': np.uint32,
          'total': np.uint64, 'best_allele': np.int32, 'best_count': np.uint32}


def run_dev(ctx, A, run_start, G=None, gene_of_run=None, abits=None, fill=0xFF, want=OUTPUTS, stream='null'):
    """allele_runs_dev on caller tensors (guard bands round every output and the workspace, garbage in them before the call)
    -> the dict of results as numpy arrays."""
    n_alleles, n_genomes = A.shape
    n_runs = len(run_start) - 1
    stride = model.stride_words(n_runs)
    sizes = {'derived': n_genomes * stride * 8, 'diff': n_genomes * stride * 8, 'diff_per_genome': n_genomes * 4,
             'diff_per_run': n_runs * 4, 'total': n_runs * 8, 'best_allele': n_runs * 4, 'best_count': n_runs * 4}
    ws_bytes = _native.lib().pgx_allele_runs_workspace_bytes(n_alleles, n_runs, n_genomes)
    assert ws_bytes > 0
    with dev.stream_scope(stream) as handle:
        d_abits = dev.upload(model.pack(A) if abits is None else abits)
        d_start = dev.upload(np.asarray(run_start, dtype=np.uint32))
        d_gbits = dev.upload(model.pack(G)) if G is not None else None
        d_gene = dev.upload(np.asarray(gene_of_run, dtype=np.int32)) if gene_of_run is not None else None
        bufs = {k: dev.guarded(sizes[k], fill) for k in want}
        ws = dev.guarded(ws_bytes, fill)
        inputs = [x for x in (d_abits, d_start, d_gbits, d_gene) if x is not None]
        with dev.unchanged(*inputs):
            ctx.allele_runs_dev(d_abits.ptr, n_alleles, d_gbits.ptr if d_gbits else None, 0 if G is None else G.shape[0],
                                n_genomes, d_start.ptr, n_runs, d_gene.ptr if d_gene else None,
                                *[bufs[k].ptr if k in bufs else None for k in OUTPUTS], ws.ptr, ws_bytes, handle)
    out = {}
    for k, b in bufs.items():
        b.assert_guards_intact()
        out[k] = b.numpy(DTYPES[k])
        if k in ('derived', 'diff'):
            out[k] = out[k].reshape(n_genomes, stride)
    ws.assert_guards_intact()
    return out


def random_runs(rng, n_alleles, n_runs, end=None):
    """n_runs + 1 sorted cut points from 0 to `end` (default n_alleles): runs of every length, empty ones included."""
    end = n_alleles if end is None else end
    cuts = np.sort(rng.integers(0, end + 1, max(n_runs - 1, 0)))
    return np.concatenate([[0], cuts, [end]]).astype(np.uint32)


def random_genes(rng, n_runs, n_genomes, derived):
    """A gene table of which most rows agree with the derived rows, and a gene_of_run with -1 and with repeats."""
    n_genes = max(1, n_runs // 2 + 1)
    gene_of_run = rng.integers(-1, n_genes, n_runs).astype(np.int32)
    G = rng.random((n_genes, n_genomes)) < 0.5
    for r in range(n_runs):
        if gene_of_run[r] >= 0 and rng.random() < 0.7:
            G[gene_of_run[r]] = derived[r]
    return G, gene_of_run


@pytest.mark.parametrize('n_alleles', (1, 63, 64, 65, 193, 4097))
def test_dev_entry_equals_the_model_at_every_size(n_alleles, gpu_ctx):
    rng = np.random.default_rng(n_alleles)
    for n_genomes in (1, 7, 64, 65):
        A = rng.random((n_alleles, n_genomes)) < rng.random((n_alleles, 1)) * 0.6
        for n_runs in sorted({1, 63, 64, 65, n_alleles}):
            run_start = random_runs(rng, n_alleles, n_runs)
            G, gene_of_run = random_genes(rng, n_runs, n_genomes, model.runs(A, run_start)['derived'])
            want = model.runs(A, run_start, G, gene_of_run)
            got = run_dev(gpu_ctx, A, run_start, G, gene_of_run, fill=dev.FILLS[(n_genomes + n_runs) % 2])
            model.assert_equal(got, want, n_runs)


def edge_layouts():
    n = 4097
    yield 'ends_at_bit_63', 130, [0, 64, 128, 130]
    yield 'starts_at_bit_0_of_a_later_word', 200, [0, 5, 128, 192, 200]
    yield 'crosses_one_word_boundary', 130, [0, 60, 70, 127, 129, 130]
    yield 'more_than_128_rows', 400, [0, 3, 3 + 190, 400]
    yield 'one_run_holds_everything', n, [0, n]
    yield 'empty_runs_front_middle_end', 193, [0, 0, 0, 64, 64, 100, 193, 193, 193]
    yield 'trailing_rows_in_no_run', 193, [0, 10, 64, 150]
    yield 'single_rows', 130, list(range(131))


LAYOUTS = list(edge_layouts())


@pytest.mark.parametrize('name,n_alleles,run_start', LAYOUTS, ids=[x[0] for x in LAYOUTS])
def test_run_layouts_that_hit_each_edge(name, n_alleles, run_start, gpu_ctx):
    rng = np.random.default_rng(len(name))
    n_runs = len(run_start) - 1
    for n_genomes, table in ((7, 'random'), (65, 'sparse'), (9, 'ones'), (9, 'zeros')):
        A = {'random': rng.random((n_alleles, n_genomes)) < 0.3, 'sparse': rng.random((n_alleles, n_genomes)) < 0.004,
             'ones': np.ones((n_alleles, n_genomes), dtype=bool), 'zeros': np.zeros((n_alleles, n_genomes), dtype=bool)}[table]
        G, gene_of_run = random_genes(rng, n_runs, n_genomes, model.runs(A, run_start)['derived'])
        gene_of_run[0] = -1
        gene_of_run[-1] = gene_of_run[n_runs // 2]                           # -1 and a repeat, whatever was drawn
        want = model.runs(A, run_start, G, gene_of_run)
        model.assert_equal(run_dev(gpu_ctx, A, run_start, G, gene_of_run, stream='side'), want, n_runs)
        # without a gene table diff = derived, and only what is asked for is written
        some = run_dev(gpu_ctx, A, run_start, want=('diff', 'best_allele'))
        assert np.array_equal(model.unpack(some['diff'], n_runs), want['derived'])
        assert np.array_equal(some['best_allele'], want['best_allele'])


def test_allele_pad_bits_are_masked_and_output_pad_bits_are_zero(gpu_ctx):
    rng = np.random.default_rng(3)
    for n_alleles, run_start in ((65, [0, 3, 65]), (193, [0, 100, 150]), (63, [0, 63]), (1, [0, 0, 1])):
        A = rng.random((n_alleles, 5)) < 0.2
        n_runs = len(run_start) - 1
        G, gene_of_run = random_genes(rng, n_runs, 5, model.runs(A, run_start)['derived'])
        want = model.runs(A, run_start, G, gene_of_run)
        dirty = model.pack(A)
        pad = np.unpackbits(np.zeros_like(dirty).view(np.uint8), axis=1, bitorder='little')
        pad[:, n_alleles:] = 1
        dirty |= np.packbits(pad, axis=1, bitorder='little').view(np.uint64)
        assert not model.pad_bits_clear(dirty, n_alleles)
        results = []
        for fill in dev.FILLS:
            got = run_dev(gpu_ctx, A, run_start, G, gene_of_run, abits=dirty, fill=fill)
            model.assert_equal(got, want, n_runs)                           # (checks the outputs' pad bits as well)
            results.append(tuple(got[k] for k in OUTPUTS))
        dev.same_bytes(results)


def test_dev_entry_reports_bad_run_arrays_and_small_workspaces(gpu_ctx):
    A = np.ones((100, 3), dtype=bool)
    G = np.ones((2, 3), dtype=bool)
    for run_start, gene_of_run, match in (([0, 50, 40, 100], [0, 0, 0], 'never decrease'), ([0, 50, 101], [0, 1], 'beyond'),
                                          ([1, 50, 100], [0, 1], 'start at 0'), ([0, 50, 100], [0, 2], 'gene_of_run'),
                                          ([0, 50, 100], [0, -2], 'gene_of_run')):
        with pytest.raises(_native.PgxError, match=match) as e:
            run_dev(gpu_ctx, A, run_start, G, gene_of_run)
        assert e.value.status == -1
    d = dev.upload(model.pack(A))
    s = dev.upload(np.array([0, 100], dtype=np.uint32))
    out = dev.guarded(4, 0xFF)
    ws = dev.guarded(256, 0xFF)
    with pytest.raises(_native.PgxError, match='workspace too small'):
        gpu_ctx.allele_runs_dev(d.ptr, 100, None, 0, 3, s.ptr, 1, None, None, None, None, out.ptr, None, None, None, ws.ptr, 256)
    with pytest.raises(_native.PgxError, match='no runs'):
        gpu_ctx.allele_runs_dev(d.ptr, 100, None, 0, 3, s.ptr, 0, None, None, None, None, out.ptr, None, None, None, ws.ptr, 256)
    gpu_ctx.allele_runs_dev(d.ptr, 100, None, 0, 3, s.ptr, 0, None, None, None, None, None, None, None, None, None, 0)
    assert out.is_still_garbage()


def coo(X):
    r, c = np.nonzero(X)
    return r.astype(np.int32), c.astype(np.int32)


def test_host_entry_equals_the_model(gpu_ctx):
    rng = np.random.default_rng(11)
    for n_alleles, n_genomes, n_runs in ((1, 1, 1), (65, 7, 64), (193, 65, 65), (4097, 64, 700), (4097, 9, 4097)):
        A = rng.random((n_alleles, n_genomes)) < 0.3
        run_start = random_runs(rng, n_alleles, n_runs, end=n_alleles - (n_alleles > 100))
        G, gene_of_run = random_genes(rng, n_runs, n_genomes, model.runs(A, run_start)['derived'])
        want = model.runs(A, run_start, G, gene_of_run)
        (ar, ac), (gr, gc) = coo(A), coo(G)
        p = rng.permutation(ar.size)
        got, dups = gpu_ctx.allele_runs(ar[p], ac[p], n_alleles, n_genomes, run_start, gr, gc, G.shape[0], gene_of_run)
        assert dups == (0, 0)
        model.assert_equal(got, want, n_runs)
        some, _ = gpu_ctx.allele_runs(ar, ac, n_alleles, n_genomes, run_start, want=('total', 'derived'))
        assert sorted(some) == ['derived', 'total']
        assert np.array_equal(some['total'], want['total'])
        assert np.array_equal(model.unpack(some['derived'], n_runs), want['derived'])


def test_host_entry_reports_duplicates_and_refuses_invalid_input(gpu_ctx):
    A = np.ones((10, 3), dtype=bool)
    G = np.ones((2, 3), dtype=bool)
    (ar, ac), (gr, gc) = coo(A), coo(G)
    ok = dict(n_alleles=10, n_genomes=3, run_start=[0, 5, 10], gene_rows=gr, gene_genomes=gc, n_genes=2, gene_of_run=[0, 1])
    out, dups = gpu_ctx.allele_runs(np.append(ar, ar[:2]), np.append(ac, ac[:2]), **ok)
    assert out is None and dups == (2, 0)
    out, dups = gpu_ctx.allele_runs(ar, ac, **dict(ok, gene_rows=np.append(gr, gr[:1]), gene_genomes=np.append(gc, gc[:1])))
    assert out is None and dups == (0, 1)
    for change, match in ((dict(run_start=[0, 6, 5, 10], gene_of_run=[0, 1, 1]), 'never decrease'),
                          (dict(run_start=[0, 5, 11]), 'beyond'), (dict(gene_of_run=[0, 2]), 'gene_of_run'),
                          (dict(run_start=[0], gene_of_run=[]), 'no runs'), (dict(run_start=[2, 5, 10]), 'start at 0')):
        with pytest.raises(_native.PgxError, match=match) as e:
            gpu_ctx.allele_runs(ar, ac, **dict(ok, **change))
        assert e.value.status == -1
    with pytest.raises(_native.PgxError, match='out of range'):
        gpu_ctx.allele_runs(np.array([10]), np.array([0]), **ok)
    out, dups = gpu_ctx.allele_runs(ar, ac, 10, 3, [0], want=())            # no runs and nothing asked for: fine
    assert out == {} and dups == (0, 0)


@pytest.mark.parametrize('as_lsdf', (False, True), ids=('frames', 'lsdf'))
@pytest.mark.parametrize('path', CASES, ids=ids)
def test_python_functions_reproduce_the_reference(path, as_lsdf, gpu_ctx, tmp_path):
    model.check_python_functions(model.load_case(path), gpu_ctx, str(tmp_path), as_lsdf)


def test_tables_of_build_cds_pangenome_are_consistent_until_an_entry_is_removed(gpu_ctx, tmp_path, golden_dir):
    src = os.path.join(golden_dir, 'cds', 'in')
    paths = sorted(os.path.join(src, f) for f in os.listdir(src) if f.endswith('.faa'))
    (tmp_path / 'out').mkdir()
    with contextlib.redirect_stdout(io.StringIO()):
        dfa, dfg = pangenome.build_cds_pangenome(paths, str(tmp_path / 'out'), name='T')
        assert pangenome.validate_gene_table(dfg, dfa, ctx=gpu_ctx) == 0
        assert pangenome.validate_gene_table_dense(dfg, dfa, ctx=gpu_ctx) == 0
        m = dfg.data
        keep = np.arange(m.nnz) != m.nnz // 2
        less = sparse_utils.LightSparseDataFrame(dfg.index, dfg.columns, scipy.sparse.coo_matrix(
            (m.data[keep], (m.row[keep], m.col[keep])), shape=m.shape))
        assert pangenome.validate_gene_table(less, dfa, ctx=gpu_ctx) == 1
        assert pangenome.validate_gene_table_dense(less, dfa, ctx=gpu_ctx) == 1
        from_file = pangenome.validate_gene_table(str(tmp_path / 'out' / 'T_strain_by_gene.npz'),
                                                  str(tmp_path / 'out' / 'T_strain_by_allele.npz'), ctx=gpu_ctx)
    assert from_file == 0


@pytest.mark.parametrize('n_genomes', (3, 70))
def test_host_entry_serves_every_output_alone_with_and_without_a_gene_table(n_genomes, gpu_ctx):
    """One output per call: each comes back through its own part of the result buffer, and diff_per_run / diff_per_genome
    alone take their diff bitmap from the workspace."""
    rng = np.random.default_rng(n_genomes)
    n_alleles, run_start = 13, np.array([0, 2, 2, 7, 12], dtype=np.uint32)       # an empty run, a last row in no run
    n_runs = run_start.size - 1
    A = rng.random((n_alleles, n_genomes)) < 0.4
    derived = model.runs(A, run_start)['derived']
    G = np.stack([~derived[0], derived[2], rng.random(n_genomes) < 0.5])         # gene 0 differs in every genome
    gene_of_run = np.array([0, -1, 1, 2], dtype=np.int32)
    (ar, ac), (gr, gc) = coo(A), coo(G)
    with_genes, without = model.runs(A, run_start, G, gene_of_run), model.runs(A, run_start)
    assert with_genes['diff'].any()
    for k in OUTPUTS:
        got, dups = gpu_ctx.allele_runs(ar, ac, n_alleles, n_genomes, run_start, gr, gc, G.shape[0], gene_of_run, want=(k,))
        assert dups == (0, 0) and list(got) == [k]
        model.assert_equal(got, {k: with_genes[k]}, n_runs)
        got, dups = gpu_ctx.allele_runs(ar, ac, n_alleles, n_genomes, run_start, want=(k,))
        assert dups == (0, 0) and list(got) == [k]
        model.assert_equal(got, {k: without[k]}, n_runs)
    got, _ = gpu_ctx.allele_runs(ar, ac, n_alleles, n_genomes, run_start, gr, gc, G.shape[0], gene_of_run,
                                 want=('diff_per_run', 'diff_per_genome'))
    model.assert_equal(got, {k: with_genes[k] for k in ('diff_per_run', 'diff_per_genome')}, n_runs)
    out, dups = gpu_ctx.allele_runs(ar, ac, n_alleles, n_genomes, [0], want=())  # no runs and nothing asked for
    assert out == {} and dups == (0, 0)
