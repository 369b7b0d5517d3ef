"""The two device steps of the proximal pangenome builders (csrc/prox.hip; include/pgx.h "The two device steps of the proximal
(5'/3' UTR) pangenome builders") against the plain-Python models of tests/prox_model.py, and the ctx= layer of
pangenomix_amd.pangenome on a real context against what the reference wrote (tests/golden/proximal, proximal_device) and
against the host path. Bytes and integers: every comparison is exact. The grouping runs twice, the second time with
PGX_PROX_NARROW_HASH: 3 bits of hash, every probe collides, same output."""
import json
import os
import shutil

import numpy as np
import pytest

import dev_entry_checks as dev
import prox_model as model
from pangenomix_amd import _native, pangenome as pg
from test_host_golden import assert_same_npz, same_file
from test_proximal_golden import GENOMES as FIRST_GENOMES, RUNS as FIRST_RUNS

pytestmark = pytest.mark.gpu

NARROW = 1                                   # PGX_PROX_NARROW_HASH
FLAGS = (0, NARROW)
LETTERS = np.frombuffer(model.LETTERS, dtype=np.uint8)


def step():
    return int(_native.lib().pgx_prox_cut_group_bytes())


def tile():
    return int(_native.lib().pgx_prox_group_tile())


def letters(rng, n):
    return LETTERS[rng.integers(0, LETTERS.size, n)].tobytes()


# -- cut ---------------------------------------------------------------------------------------------------------------------
def check_cut(ctx, text, start, length, reverse):
    want_out, want_off, want_bad = model.cut(text, start, length, reverse)
    out, off, bad = ctx.prox_cut(text, start, length, reverse)
    assert out.dtype == np.uint8 and bad.dtype == np.uint8 and off.dtype == np.uint64
    assert np.array_equal(off, want_off)
    assert np.array_equal(bad, want_bad), 'bad differs at %r' % np.flatnonzero(bad != want_bad)[:10].tolist()
    assert out.tobytes() == want_out, 'out differs first at byte %d' % int(
        np.flatnonzero(out != np.frombuffer(want_out, dtype=np.uint8))[0])
    return out, off, bad


def test_cut_lengths_at_every_alignment(gpu_ctx):
    S = step()
    assert S % 16 == 0 and S >= 16
    lengths = sorted({0, 1, 15, 16, 17, 31, 32, 33, 53, 255, 256, 257, S - 1, S, S + 1})
    rng = np.random.default_rng(1)
    text = letters(rng, 2 * S + 600)
    start, length, reverse = [], [], []
    for n in lengths:
        for a in range(16):
            for r in (0, 1):
                # every start alignment; the windows of one length follow each other in the output, so the alignment of
                # the piece written moves as well
                start += [32 + a, 0, len(text) - n]              # ... at offset 0 and ending at the last byte
                length += [n] * 3
                reverse += [r] * 3
    out, off, bad = check_cut(gpu_ctx, text, start, length, reverse)
    assert not bad.any() and len({int(o) % 16 for o in off}) == 16


@pytest.mark.parametrize('n', (0, 1, 63, 64, 65, 1000, 20000))
def test_cut_window_counts_overlapping_and_identical(n, gpu_ctx):
    rng = np.random.default_rng(n)
    text = letters(rng, 5000)
    length = rng.integers(0, 90, n)
    start = rng.integers(0, len(text) - 90, n)
    reverse = rng.integers(0, 2, n)
    if n >= 63:
        start[10:20] = start[10]                                 # identical windows, and the same span in both directions
        length[10:20] = 53
        reverse[10:20:2] = 1
        start[30:40] = start[30] + np.arange(10)                 # overlapping, a byte apart
    out, off, bad = check_cut(gpu_ctx, text, start, length, reverse)
    assert out.size == int(length.sum()) and bad.size == n


def test_cut_forward_takes_any_byte_and_reverse_only_the_table(gpu_ctx):
    rng = np.random.default_rng(3)
    alphabet = np.array([0x00, 0x7f, 0x80, 0xff], dtype=np.uint8)
    text = alphabet[rng.integers(0, 4, 700)].tobytes()
    start = rng.integers(0, 600, 200)
    length = rng.integers(0, 100, 200)
    out, off, bad = check_cut(gpu_ctx, text, start, length, np.zeros(200, dtype=np.uint8))
    assert not bad.any() and {0x00, 0x7f, 0x80, 0xff} <= set(out.tolist())
    # each letter of the table on its own, and in one window
    table = model.LETTERS
    out, off, bad = check_cut(gpu_ctx, table, list(range(22)) + [0], [1] * 22 + [22], [1] * 23)
    assert out[:22].tobytes() == b'TGCAWSYRKMNtgcawsyrkmn' and not bad.any()
    # every byte value alone in a reverse window: exactly the 22 letters have a complement
    every = bytes(range(256))
    out, off, bad = check_cut(gpu_ctx, every, list(range(256)), [1] * 256, [1] * 256)
    assert int((bad == 0).sum()) == 22 and (out[bad == 1] == 0).all()


@pytest.mark.parametrize('n', (1, 16, 17, 53, 257))
def test_cut_one_bad_byte_in_a_reverse_window(n, gpu_ctx):
    """bad is set for that window alone, a 0 is written where the byte goes, the neighbouring windows are untouched"""
    rng = np.random.default_rng(n)
    for at in sorted({0, n // 2, n - 1}):
        for bad_byte in (ord('X'), 0x00, 0xff, ord('\n')):
            text = bytearray(letters(rng, 3 * n + 40))
            text[20 + n + at] = bad_byte
            start, length = [20, 20 + n, 20 + 2 * n, 20 + n], [n] * 4
            out, off, bad = check_cut(gpu_ctx, bytes(text), start, length, [1, 1, 1, 0])
            assert bad.tolist() == [0, 1, 0, 0]
            assert out[n + (n - 1 - at)] == 0 and int((out == 0).sum()) == (2 if bad_byte == 0 else 1)


def test_cut_smallest_texts(gpu_ctx):
    check_cut(gpu_ctx, b'A', [0, 0, 1, 0], [1, 1, 0, 0], [0, 1, 1, 0])
    out, off, bad = gpu_ctx.prox_cut(b'', [0, 0], [0, 0], [0, 1])
    assert out.size == 0 and off.tolist() == [0, 0, 0] and bad.tolist() == [0, 0]
    out, off, bad = gpu_ctx.prox_cut(b'ACGT', [], [], [])
    assert out.size == 0 and off.tolist() == [0] and bad.size == 0


def cut_dev_case(seed, n=400):
    rng = np.random.default_rng(seed)
    text = bytearray(letters(rng, 3000))
    for at in rng.integers(0, 3000, 12):
        text[int(at)] = 0x80                                     # some bad windows
    length = rng.integers(0, 2 * step() + 20, n).astype(np.uint32)
    length[::7] = 53
    start = rng.integers(0, 3000 - int(length.max()), n).astype(np.uint64)
    start[0] = 0                                                 # a window at offset 0 ...
    start[-1] = 3000 - int(length[-1])                            # ... and one that ends at the last byte
    reverse = rng.integers(0, 2, n).astype(np.uint8)
    return bytes(text), start, length, reverse


def run_cut_dev(ctx, text, start, length, reverse, fill, stream, shift=0):
    """shift: text and output start `shift` bytes off 16-byte alignment, the text at the very end of its allocation"""
    import torch
    start, length, reverse = np.asarray(start, dtype=np.uint64), np.asarray(length, dtype=np.uint32), np.asarray(reverse, dtype=np.uint8)
    want_out, off, want_bad = model.cut(text, start, length, reverse)
    n = len(start)
    with dev.stream_scope(stream) as handle:
        g_text = dev.guarded(shift + len(text), 0x5A)
        g_text.raw[dev.GUARD + shift:dev.GUARD + shift + len(text)] = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
        d_start, d_length, d_reverse, d_off = dev.upload(start), dev.upload(length), dev.upload(reverse), dev.upload(off)
        # (the payload ends 16 - shift bytes after the output: what is left of the last aligned word stays as it was)
        out, bad = dev.guarded(shift + len(want_out) + (16 - shift) % 16, fill), dev.guarded(n, fill)
        with dev.unchanged(d_start, d_length, d_reverse, d_off, g_text.raw):
            ctx.prox_cut_dev(g_text.ptr + shift, len(text), d_start.ptr, d_length.ptr, d_reverse.ptr, d_off.ptr, n,
                             out.ptr + shift, bad.ptr, handle)
    out.assert_guards_intact()
    bad.assert_guards_intact()
    raw = out.numpy(np.uint8)
    assert (raw[:shift] == fill).all() and (raw[shift + len(want_out):] == fill).all(), 'bytes beside the output were written'
    got = raw[shift:shift + len(want_out)], bad.numpy(np.uint8)
    assert got[0].tobytes() == want_out and np.array_equal(got[1], want_bad)
    return got


@pytest.mark.parametrize('stream', dev.STREAMS)
def test_cut_device_entry_on_caller_tensors(stream, gpu_ctx):
    for seed, n in ((1, 400), (2, 1), (3, 65)):
        case = cut_dev_case(seed, n)
        dev.same_bytes([run_cut_dev(gpu_ctx, *case, fill, stream) for fill in dev.FILLS])


def test_cut_device_entry_off_16_byte_alignment(gpu_ctx):
    case = cut_dev_case(4)
    for shift in (1, 15, 8):
        run_cut_dev(gpu_ctx, *case, 0x5A, 'null', shift=shift)
    run_cut_dev(gpu_ctx, b'G', [0, 0], [1, 1], [1, 0], 0xFF, 'null', shift=5)          # a text of one byte


def test_cut_device_entry_does_not_allocate(gpu_ctx):
    text, start, length, reverse = cut_dev_case(5)
    want_out, off, _ = model.cut(text, start, length, reverse)
    d = [dev.upload(np.frombuffer(text, dtype=np.uint8)), dev.upload(start), dev.upload(length), dev.upload(reverse), dev.upload(off)]
    out, bad = dev.guarded(len(want_out), 0xFF), dev.guarded(len(start), 0xFF)
    dev.assert_no_allocation(lambda: gpu_ctx.prox_cut_dev(d[0].ptr, len(text), d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr,
                                                          len(start), out.ptr, bad.ptr))
    assert out.numpy(np.uint8).tobytes() == want_out


# -- group -------------------------------------------------------------------------------------------------------------------
def check_group(ctx, records, genes, flags, lead=0):
    want = model.group(records, genes)
    blob, off = model.blob(records, lead)
    first, variant, distinct = ctx.prox_group(blob, off, genes, flags=flags)
    assert first.dtype == np.int32 and variant.dtype == np.int32
    assert np.array_equal(first, want[0]), 'first differs at %r' % np.flatnonzero(first != want[0])[:10].tolist()
    assert np.array_equal(variant, want[1]), 'variant differs at %r' % np.flatnonzero(variant != want[1])[:10].tolist()
    assert distinct == want[2]
    again = ctx.prox_group(blob, off, genes, flags=flags)                        # two calls, identical bytes
    assert again[0].tobytes() == first.tobytes() and again[1].tobytes() == variant.tobytes() and again[2] == distinct
    return first, variant, distinct


@pytest.mark.parametrize('flags', FLAGS)
def test_group_what_makes_two_records_equal(flags, gpu_ctx):
    rng = np.random.default_rng(1)
    a = letters(rng, 53)
    near = [a[:-1] + bytes([a[-1] ^ 1]), a[:-1], a + a[-1:], a + b'\x00', bytes([a[0] ^ 1]) + a[1:], a[:16], a[:17]]
    records = [a, a, a] + near + [a] + near + [b'', b'', b'\x00', b'']
    genes = [3, 4, 3] + [3] * len(near) + [4] + [3] * len(near) + [3, 4, 3, 3]
    first, variant, distinct = check_group(gpu_ctx, records, genes, flags)
    assert first[:3].tolist() == [0, 1, 0] and variant[:3].tolist() == [0, 0, 0]       # the same bytes under two genes
    assert variant[3:3 + len(near)].tolist() == list(range(1, len(near) + 1))            # last byte only, length only, ...
    assert first[-4:].tolist() == [len(records) - 4, len(records) - 3, len(records) - 2, len(records) - 4]
    assert distinct == 2 + len(near) + 3
    # every record equal; every record empty
    for same in (a, b''):
        first, variant, distinct = check_group(gpu_ctx, [same] * 130, [7] * 130, flags)
        assert not first.any() and not variant.any() and distinct == 1


@pytest.mark.parametrize('flags', FLAGS)
@pytest.mark.parametrize('n', (0, 1, 2, 63, 64, 65, 1000, 20000))
def test_group_record_counts(n, flags, gpu_ctx):
    """about a third of the records repeat an earlier one of their gene; equal records adjacent and n - 1 apart"""
    rng = np.random.default_rng(n)
    pool = [letters(rng, int(k)) for k in rng.integers(0, 80, max(n // 3, 1))]
    records = [pool[int(i)] for i in rng.integers(0, len(pool), n)]
    genes = rng.integers(0, max(n // 20, 1), n).tolist()
    if n >= 2:
        records[-1], genes[-1] = records[0], genes[0]                            # n - 1 apart (19,999 at the largest)
    if n >= 63:
        records[41], genes[41] = records[40], genes[40]                          # adjacent
    first, variant, distinct = check_group(gpu_ctx, records, genes, flags)
    assert first.size == n and (n < 2 or first[-1] == first[0])
    if n >= 63:
        assert 0 < distinct < n


@pytest.mark.parametrize('flags', FLAGS)
def test_group_one_gene_with_20000_distinct_windows(flags, gpu_ctx):
    rng = np.random.default_rng(5)
    records = list({letters(rng, 53) for _ in range(20400)})[:20000]
    assert len(records) == 20000
    first, variant, distinct = check_group(gpu_ctx, records, [9] * 20000, flags)
    assert np.array_equal(variant, np.arange(20000)) and distinct == 20000


@pytest.mark.parametrize('flags', FLAGS)
def test_group_20000_genes_of_one_record_each(flags, gpu_ctx):
    rng = np.random.default_rng(6)
    same = letters(rng, 53)
    genes = np.arange(20000) * 800                                               # spread over all three digits of the sort
    genes[-1] = (1 << 24) - 1                                                    # the smallest and the largest gene id
    genes = rng.permutation(genes)
    first, variant, distinct = check_group(gpu_ctx, [same] * 20000, genes.tolist(), flags)
    assert np.array_equal(first, np.arange(20000)) and not variant.any() and distinct == 20000


@pytest.mark.parametrize('flags', FLAGS)
def test_group_firsts_on_both_sides_of_every_boundary_of_the_sort(flags, gpu_ctx):
    """a gene's variants are numbered across the tiles of the sort, the tiles of the scans and the digits of the gene id:
    firsts sit right before and right after every such index, duplicates of them everywhere else"""
    T = tile()
    n = 4 * T + 37
    edges = sorted({x for b in (64, 256, T, 2048, 2 * T, 3 * T, 4 * T) for x in (b - 1, b, b + 1) if x < n} | {0, n - 1})
    digit_genes = [0, 1, 255, 256, 257, 65535, 65536, 65537, (1 << 24) - 1]
    rng = np.random.default_rng(7)
    for spread in (False, True):
        records, genes = [None] * n, [None] * n
        for k, at in enumerate(edges):
            records[at] = b'edge%d' % k + letters(rng, 20)
            genes[at] = digit_genes[k % len(digit_genes)] if spread else 256
        for at in range(n):
            if records[at] is None:
                src = edges[int(rng.integers(0, len(edges)))]                    # a copy of an edge record: of a later one too,
                records[at], genes[at] = records[src], genes[src]                # which makes this copy the first
        first, variant, distinct = check_group(gpu_ctx, records, genes, flags)
        assert distinct == len(edges)


def group_dev_case(seed, n=700):
    rng = np.random.default_rng(seed)
    pool = [letters(rng, int(k)) for k in rng.integers(0, 2 * step() + 20, max(n // 2, 1))]
    records = [pool[int(i)] for i in rng.integers(0, len(pool), n)]
    genes = rng.choice([0, 5, 255, 256, 70000, (1 << 24) - 1], n).astype(np.int32)
    return records, genes


def run_group_dev(ctx, records, genes, flags, fill, stream, lead=0, shift=0):
    import torch
    want = model.group(records, genes.tolist())
    blob, off = model.blob(records, lead)
    n = len(records)
    ws_bytes = ctx.prox_group_workspace_bytes(n)
    assert ws_bytes > 0
    with dev.stream_scope(stream) as handle:
        g_blob = dev.guarded(shift + blob.size, 0x5A)
        g_blob.raw[dev.GUARD + shift:dev.GUARD + shift + blob.size] = torch.from_numpy(blob.copy()).cuda()
        d_off, d_gene = dev.upload(off), dev.upload(genes)
        first, variant, distinct, ws = (dev.guarded(4 * n, fill), dev.guarded(4 * n, fill), dev.guarded(4, fill),
                                        dev.guarded(ws_bytes, fill))
        with dev.unchanged(d_off, d_gene, g_blob.raw):
            ctx.prox_group_dev(g_blob.ptr + shift, d_off.ptr, d_gene.ptr, n, first.ptr, variant.ptr, distinct.ptr, ws.ptr,
                               ws_bytes, flags, handle)
    for buf in (first, variant, distinct, ws):
        buf.assert_guards_intact()
    got = first.numpy(np.int32), variant.numpy(np.int32), distinct.numpy(np.uint32)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2].tolist() == [want[2]]
    return got


@pytest.mark.parametrize('flags', FLAGS)
@pytest.mark.parametrize('stream', dev.STREAMS)
def test_group_device_entry_on_caller_tensors(stream, flags, gpu_ctx):
    for seed, n in ((1, 700), (2, 1), (3, 65), (4, 2 * tile() + 3)):
        case = group_dev_case(seed, n)
        dev.same_bytes([run_group_dev(gpu_ctx, *case, flags, fill, stream) for fill in dev.FILLS])
    run_group_dev(gpu_ctx, *group_dev_case(5), flags, 0xFF, stream, lead=7)
    for shift in (1, 15, 8):                                                     # a blob off 16-byte alignment
        run_group_dev(gpu_ctx, *group_dev_case(6), flags, 0x5A, stream, shift=shift)


def test_group_device_entry_does_not_allocate(gpu_ctx):
    records, genes = group_dev_case(7)
    blob, off = model.blob(records)
    n, ws_bytes = len(records), gpu_ctx.prox_group_workspace_bytes(len(records))
    d_blob, d_off, d_gene = dev.upload(blob), dev.upload(off), dev.upload(genes)
    first, variant, distinct, ws = dev.guarded(4 * n, 0xFF), dev.guarded(4 * n, 0xFF), dev.guarded(4, 0xFF), dev.guarded(ws_bytes, 0xFF)
    dev.assert_no_allocation(lambda: gpu_ctx.prox_group_dev(d_blob.ptr, d_off.ptr, d_gene.ptr, n, first.ptr, variant.ptr,
                                                            distinct.ptr, ws.ptr, ws_bytes))
    assert np.array_equal(first.numpy(np.int32), model.group(records, genes.tolist())[0])


def test_invalid_calls_are_refused_before_anything_is_written(gpu_ctx):
    lib, P, h = _native.lib(), _native._ptr, gpu_ctx._h
    text = np.frombuffer(b'ACGTACGT', dtype=np.uint8)
    start, length, reverse = np.array([0, 4], dtype=np.uint64), np.array([4, 4], dtype=np.uint32), np.zeros(2, dtype=np.uint8)
    out, bad = np.full(16, 0x6E, dtype=np.uint8), np.full(2, 0x6E, dtype=np.uint8)
    first, variant = np.full(3, 0x6E6E6E6E, dtype=np.int32), np.full(3, 0x6E6E6E6E, dtype=np.int32)
    distinct = np.full(1, 0x6E6E6E6E, dtype=np.uint32)

    def refused(rc, who):
        assert rc == -1, who                                                     # PGX_ERR_INVALID
        assert (out == 0x6E).all() and (bad == 0x6E).all() and (first == 0x6E6E6E6E).all(), who
        assert (variant == 0x6E6E6E6E).all() and (distinct == 0x6E6E6E6E).all(), who
    cut = lambda s, n_len, n=2, tb=8: lib.pgx_prox_cut(h, P(text), tb, P(s), P(n_len), P(reverse), n, P(out), P(bad))   # noqa: E731
    refused(cut(np.array([0, 5], dtype=np.uint64), length), 'a window runs past the end')
    refused(cut(np.array([0, 9], dtype=np.uint64), np.array([4, 0], dtype=np.uint32)), 'a window starts past the end')
    refused(cut(np.array([0, (1 << 64) - 2], dtype=np.uint64), length), 'start + length wraps')
    refused(cut(start, length, tb=1 << 32), 'text_bytes')
    refused(cut(start, length, n=1 << 24), 'n')
    assert cut(start, length) == 0 and out[:8].tobytes() == b'ACGTACGT' and bad.tolist() == [0, 0]
    out[:], bad[:] = 0x6E, 0x6E
    blob, off = model.blob([b'AC', b'GT', b'A'])
    gene = np.array([0, 1, 0], dtype=np.int32)
    group = lambda o, g, n=3, flags=0: lib.pgx_prox_group(h, P(blob), P(o), P(g), n, flags, P(first), P(variant), P(distinct))   # noqa: E731
    refused(group(off, gene, n=1 << 24), 'n')
    refused(group(off, gene, flags=2), 'flags')
    down, big = off.copy(), off.copy()
    down[2], big[3] = 1, 1 << 32
    refused(group(down, gene), 'decreasing offsets')
    refused(group(big, gene), 'a blob of 2^32 bytes')
    refused(group(off, np.array([0, -1, 0], dtype=np.int32)), 'a negative gene')
    refused(group(off, np.array([0, 1 << 24, 0], dtype=np.int32)), 'a gene of 2^24')
    assert lib.pgx_prox_group_workspace_bytes(1 << 24) == 0 and lib.pgx_prox_group_workspace_bytes(0) > 0
    assert group(off, gene) == 0 and first.tolist() == [0, 1, 2] and distinct.tolist() == [3]
    # the device entries refuse the same without touching their buffers
    g = dev.guarded(4096, 0x5A)
    ws_bytes = gpu_ctx.prox_group_workspace_bytes(3)
    for n, flags, ws in ((1 << 24, 0, 1 << 30), (3, 2, ws_bytes), (3, 0, ws_bytes - 8), (3, 0, 0)):
        with pytest.raises(_native.PgxError) as e:
            gpu_ctx.prox_group_dev(g.ptr, g.ptr, g.ptr, n, g.ptr, g.ptr, g.ptr, g.ptr, ws, flags)
        assert e.value.status == -1
    for n, tb in ((1 << 24, 8), (2, 1 << 32)):
        with pytest.raises(_native.PgxError) as e:
            gpu_ctx.prox_cut_dev(g.ptr, tb, g.ptr, g.ptr, g.ptr, g.ptr, n, g.ptr, g.ptr)
        assert e.value.status == -1
    assert g.is_still_garbage()
    g.assert_guards_intact()


# -- the Python layer on a real context --------------------------------------------------------------------------------------
RECORDED = model.recorded_runs(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))


@pytest.mark.parametrize('tag', sorted(RECORDED))
def test_builders_equal_the_reference_on_the_recorded_runs(tag, gpu_ctx, tmp_path, golden_dir, capsys):
    """files, .npz members, labels, stdout, exceptions and partial files, the path counts, and a second call on the
    extracts the first one left"""
    model.run_recorded(RECORDED[tag], gpu_ctx, tmp_path, golden_dir, capsys)


@pytest.mark.parametrize('tag', sorted(FIRST_RUNS))
def test_builders_equal_the_reference_on_the_first_fixtures(tag, gpu_ctx, tmp_path, golden_dir, capsys):
    fn, kw, name, side, footer = FIRST_RUNS[tag]
    din = tmp_path / 'in'
    shutil.copytree(os.path.join(golden_dir, 'proximal', 'in'), din)
    exp = os.path.join(golden_dir, 'proximal', 'expected', tag)
    (tmp_path / 'out').mkdir()
    pairs = [(str(din / (g + '.gff')), str(din / (g + '.fna'))) for g in FIRST_GENOMES]
    for call in (1, 2):                                                          # the second one on pre-existing extracts
        capsys.readouterr()
        pg.PROXIMAL_PATH_COUNTS.clear()
        df = fn(pairs, str(din / 'T_allele_names.tsv'), str(tmp_path / 'out'), ctx=gpu_ctx, **kw)
        printed = capsys.readouterr().out.replace(str(din), '<in>').replace(str(tmp_path / 'out'), '<out>')
        if call == 1:
            assert printed == json.load(open(os.path.join(golden_dir, 'proximal', 'expected', 'stdout.json')))[tag]
            assert dict(pg.PROXIMAL_PATH_COUNTS) == {'extract_device': 3, 'consolidate_device': 1}
        else:
            assert printed.count('Using pre-existing') == 3 and dict(pg.PROXIMAL_PATH_COUNTS) == {'consolidate_device': 1}
        for g in FIRST_GENOMES:
            f = '%s_%s%s.fna' % (g, side, footer)
            same_file(str(din / 'derived' / f), os.path.join(exp, f))
        same_file(str(tmp_path / 'out' / ('%s_nr_%s.fna' % (name, side))), os.path.join(exp, '%s_nr_%s.fna' % (name, side)))
        npz = '%s_strain_by_%s.npz' % (name, side)
        same_file(str(tmp_path / 'out' / (npz + '.labels.txt')), os.path.join(exp, npz + '.labels.txt'))
        assert_same_npz(str(tmp_path / 'out' / npz), os.path.join(exp, npz))
        assert list(df.columns) == ['p10', 'p1', 'p2']


def test_builders_equal_the_host_path_on_generated_genomes(gpu_ctx, tmp_path, capsys):
    model.compare_with_host_path(gpu_ctx, tmp_path, capsys)


@pytest.mark.parametrize('n', (1, 3, 70))
def test_cut_windows_that_are_all_empty(n, gpu_ctx):
    """every length 0 on a text that is not empty: no output byte, the offsets all 0, no window bad"""
    rng = np.random.default_rng(n)
    text = letters(rng, 40)
    out, off, bad = check_cut(gpu_ctx, text, rng.integers(0, 41, n).tolist(), [0] * n, rng.integers(0, 2, n).tolist())
    assert len(bytes(out)) == 0 and not np.asarray(off).any() and not np.asarray(bad).any()
