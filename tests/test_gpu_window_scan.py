"""The window scan on the device (csrc/scan.hip; include/pgx.h "Exact search for fixed-length keys") against
the set-of-slices model (tests/window_scan_model.py), and the three validators of pangenomix_amd.pangenome built on it against
what the reference printed and raised (tests/golden/proximal_direct). Bytes and integers: every comparison is exact.
Everything runs twice, the second time with PGX_SCAN_NARROW_HASH: 3 bits of hash, every probe collides, same output."""
import numpy as np
import pytest

import dev_entry_checks as dev
import window_scan_model as model
from pangenomix_amd import _native, pangenome as pg

pytestmark = pytest.mark.gpu

NARROW = 1                                   # PGX_SCAN_NARROW_HASH
FLAGS = (0, NARROW)
WINDOWS = (1, 2, 3, 4, 5, 7, 8, 53, 64, 65, 255, 1024)
CASES = model.load_cases()


def tile():
    return int(_native.lib().pgx_window_scan_tile())


def text_sizes(window, T):
    return sorted({0, 1, window - 1, window, window + 1, T - 1, T, T + 1, 2 * T + window - 2, 3 * T + 5})


def check(ctx, text, keys, flags):
    window = keys.shape[1]
    want = model.scan(text, keys, window)
    got = ctx.window_scan(text, keys, flags)
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want), 'keys %r differ' % np.flatnonzero(got != want)[:10].tolist()
    return want


@pytest.mark.parametrize('flags', FLAGS)
@pytest.mark.parametrize('window', WINDOWS)
def test_kernel_equals_the_model_at_every_text_size(window, flags, gpu_ctx):
    T = tile()
    assert T >= 1024 and T % 16 == 0
    hits = 0
    for text_bytes in text_sizes(window, T):
        # the full byte alphabet: a near miss is a miss; four letters: repeats, chance matches and long common prefixes
        for alphabet in ((None,) if window > 8 else (None, b'ACGT')):
            text, keys = model.kernel_case(window, text_bytes, T, alphabet=alphabet)
            want = check(gpu_ctx, text, keys, flags)
            hits += int(want.sum())
            if text_bytes < window:
                assert not want.any()
    assert hits > 0


@pytest.mark.parametrize('flags', FLAGS)
@pytest.mark.parametrize('n_keys', (0, 1, 2, 63, 64, 65, 1000, 20000))
def test_key_counts(n_keys, flags, gpu_ctx):
    """20000 keys are past anything a table in LDS alone would hold"""
    T, window = tile(), 12
    rng = np.random.default_rng(n_keys)
    text = rng.integers(0, 256, T + 777, dtype=np.uint8)
    starts = rng.integers(0, text.size - window + 1, n_keys)
    keys = np.stack([text[s:s + window] for s in starts]) if n_keys else np.zeros((0, window), dtype=np.uint8)
    keys = keys.copy()
    absent = rng.random(n_keys) < 0.5
    keys[absent, rng.integers(0, window, int(absent.sum()))] ^= 0x40
    want = check(gpu_ctx, text, keys, flags)
    assert n_keys < 63 or (0 < want.sum() < n_keys)


@pytest.mark.parametrize('flags', FLAGS)
def test_key_properties(flags, gpu_ctx):
    T = tile()
    rng = np.random.default_rng(5)
    text = rng.choice(np.array([0x00, 0x7f, 0x80, 0xff, ord('a'), ord('A')], dtype=np.uint8), T + 300)
    text[100:105] = np.frombuffer(b'aAaAa', dtype=np.uint8)
    window = 5
    keys = [text[100:105], text[100:105],                       # equal keys: both flagged
            np.frombuffer(b'AaAaA', dtype=np.uint8),             # a against A
            np.frombuffer(b'aAaAb', dtype=np.uint8),             # absent
            np.array([0x00] * 5, dtype=np.uint8), np.array([0xff] * 5, dtype=np.uint8),
            np.array([0x80, 0x7f, 0x80, 0x7f, 0x00], dtype=np.uint8), np.array([0x7f, 0x80, 0xff, 0x00, 0x80], dtype=np.uint8),
            text[T - 2:T + 3], text[T - 2:T + 3], text[-5:], text[:5]]
    keys = np.stack(keys)
    want = check(gpu_ctx, text, keys, flags)
    assert want[0] == want[1] == 1 and want[3] == 0 and want[8] == want[9] == 1 and want[10] == want[11] == 1
    # every position matches every key: a text and keys of one repeated byte
    same = np.full(2 * T + 9, 0x80, dtype=np.uint8)
    assert check(gpu_ctx, same, np.full((3, 64), 0x80, dtype=np.uint8), flags).all()
    assert not check(gpu_ctx, same, np.full((3, 64), 0x00, dtype=np.uint8), flags).any()


def test_invalid_calls_are_refused_before_anything_is_written(gpu_ctx):
    lib = _native.lib()
    text = np.frombuffer(b'ACGTACGT', dtype=np.uint8).copy()
    keys = np.zeros((2, 1025), dtype=np.uint8)
    for text_bytes, window, n_keys in ((8, 0, 2), (8, 1025, 2), (1 << 32, 4, 2), (8, 4, 1 << 24)):
        found = np.full(2, 0xEE, dtype=np.uint8)
        rc = lib.pgx_window_scan(gpu_ctx._h, _native._ptr(text), text_bytes, _native._ptr(keys), n_keys, window, 0,
                                 _native._ptr(found))
        assert rc == -1, (text_bytes, window, n_keys)                   # PGX_ERR_INVALID
        assert lib.pgx_last_error().decode().startswith('scan_args')
        assert (found == 0xEE).all()
        assert lib.pgx_window_scan_workspace_bytes(text_bytes, n_keys, window) == 0
    with pytest.raises(_native.PgxError, match='flags'):
        gpu_ctx.window_scan(text, keys[:, :4], flags=2)
    # the device entry refuses the same sizes without touching its buffers
    out = dev.guarded(2, 0x5A)
    for text_bytes, window in ((8, 0), (8, 1025), (1 << 32, 4)):
        with pytest.raises(_native.PgxError) as e:
            gpu_ctx.window_scan_dev(out.ptr, text_bytes, out.ptr, 2, window, out.ptr, out.ptr, 1 << 20)
        assert e.value.status == -1
    assert out.is_still_garbage()
    out.assert_guards_intact()
    # legal degenerate calls
    assert gpu_ctx.window_scan(text, np.zeros((0, 4), dtype=np.uint8)).shape == (0,)
    assert not gpu_ctx.window_scan(np.zeros(0, dtype=np.uint8), text.reshape(2, 4)).any()


def run_dev(ctx, text, keys, flags, fill, stream):
    n_keys, window = keys.shape
    ws_bytes = _native.lib().pgx_window_scan_workspace_bytes(text.size, n_keys, window)
    assert ws_bytes > 0
    with dev.stream_scope(stream) as handle:
        d_text, d_keys = dev.upload(text), dev.upload(keys)
        found, ws = dev.guarded(n_keys, fill), dev.guarded(ws_bytes, fill)
        with dev.unchanged(d_text, d_keys):
            ctx.window_scan_dev(d_text.ptr, text.size, d_keys.ptr, n_keys, window, found.ptr, ws.ptr, ws_bytes, flags, handle)
    found.assert_guards_intact()
    ws.assert_guards_intact()
    return found.numpy(np.uint8)


@pytest.mark.parametrize('flags', FLAGS)
@pytest.mark.parametrize('stream', dev.STREAMS)
def test_device_entry_on_caller_tensors(stream, flags, gpu_ctx):
    T = tile()
    results = []
    for text_bytes, window in ((2 * T + 51, 53), (T + 1, 1024), (7, 8), (0, 3), (3 * T + 5, 1)):
        text, keys = model.kernel_case(window, text_bytes, T, seed=1)
        want = model.scan(text, keys, window)
        per_fill = []
        for fill in dev.FILLS:                                        # found and the workspace pre-filled with garbage
            got = run_dev(gpu_ctx, text, keys, flags, fill, stream)
            assert set(np.unique(got).tolist()) <= {0, 1}
            assert np.array_equal(got, want)
            per_fill.append((got,))
        results.append(dev.same_bytes(per_fill))
    assert any(r[0].any() for r in results)


def test_device_entry_text_that_is_not_16_byte_aligned(gpu_ctx):
    """a text that starts anywhere inside a caller's buffer: the tile loads fall back to bytes"""
    import torch
    T, window = tile(), 53
    text, keys = model.kernel_case(window, 2 * T + 100, T, seed=2)
    want = model.scan(text, keys, window)
    ws_bytes = _native.lib().pgx_window_scan_workspace_bytes(text.size, keys.shape[0], window)
    for shift in (1, 4, 15):
        buf = torch.zeros(shift + text.size, dtype=torch.uint8, device='cuda')
        buf[shift:] = torch.from_numpy(text).cuda()
        d_keys = dev.upload(keys)
        found, ws = dev.guarded(keys.shape[0], 0xFF), dev.guarded(ws_bytes, 0xFF)
        torch.cuda.synchronize()
        gpu_ctx.window_scan_dev(buf.data_ptr() + shift, text.size, d_keys.ptr, keys.shape[0], window, found.ptr, ws.ptr, ws_bytes)
        assert np.array_equal(found.numpy(np.uint8), want)
        found.assert_guards_intact()


def test_device_entry_does_not_allocate(gpu_ctx):
    T, window = tile(), 53
    text, keys = model.kernel_case(window, T + 9, T, seed=3)
    ws_bytes = _native.lib().pgx_window_scan_workspace_bytes(text.size, keys.shape[0], window)
    d_text, d_keys = dev.upload(text), dev.upload(keys)
    found, ws = dev.guarded(keys.shape[0], 0xFF), dev.guarded(ws_bytes, 0xFF)
    dev.assert_no_allocation(lambda: gpu_ctx.window_scan_dev(d_text.ptr, text.size, d_keys.ptr, keys.shape[0], window, found.ptr,
                                                             ws.ptr, ws_bytes))


@pytest.mark.parametrize('table', ('frame', 'lsdf'))
@pytest.mark.parametrize('name', sorted(CASES))
def test_validators_equal_the_reference(name, table, gpu_ctx, capsys):
    """stdout (paths normalised), return value and exceptions; an LSDF and a pandas frame give the same"""
    case = CASES[name]
    df = model.case_frame(case) if table == 'frame' else model.case_lsdf(case)
    printed, result, exc = model.run_validator(pg.validate_proximal_table_direct, case, df, capsys, limits=tuple(case['limits']),
                                               side=case['side'], log_group=case['log_group'], ctx=gpu_ctx)
    model.assert_as_recorded(case, printed, result, exc)


def test_wrappers_equal_the_direct_call_with_their_default_limits(gpu_ctx, capsys):
    for fn, side, limits, names in (
            (pg.validate_upstream_table_direct, 'upstream', (-50, 3),
             ('up_consistent_lg1', 'up_consistent_lg2', 'up_two_genes_share_a_sequence', 'contig_with_unknown_bases')),
            (pg.validate_downstream_table_direct, 'downstream', (-3, 50),
             ('down_consistent_lg1', 'down_consistent_lg2', 'genome_absent_from_the_table'))):
        for name in names:
            case = CASES[name]
            assert tuple(case['limits']) == limits and case['side'] == side
            wrapped = model.run_validator(fn, case, model.case_lsdf(case), capsys, log_group=case['log_group'], ctx=gpu_ctx)
            direct = model.run_validator(pg.validate_proximal_table_direct, case, model.case_lsdf(case), capsys, limits=limits,
                                         side=side, log_group=case['log_group'], ctx=gpu_ctx)
            model.assert_as_recorded(case, *wrapped)
            assert wrapped[:2] == direct[:2] and type(wrapped[2]) is type(direct[2])


def test_validator_on_the_table_the_builder_returns(gpu_ctx, golden_dir, tmp_path, capsys):
    """build_upstream_pangenome's LSDF goes straight into validate_upstream_table_direct: nothing is missing"""
    import os
    import shutil
    din = tmp_path / 'in'
    shutil.copytree(os.path.join(golden_dir, 'proximal', 'in'), din)
    (tmp_path / 'out').mkdir()
    genomes = ['p1', 'p2', 'p10']
    pairs = [(str(din / (g + '.gff')), str(din / (g + '.fna'))) for g in genomes]
    df = pg.build_upstream_pangenome(pairs, str(din / 'T_allele_names.tsv'), str(tmp_path / 'out'))
    capsys.readouterr()
    missing = pg.validate_upstream_table_direct(df, [p[1] for p in pairs], str(tmp_path / 'out' / 'Test_nr_upstream.fna'),
                                                ctx=gpu_ctx)
    printed = capsys.readouterr().out.replace(str(din), '<golden>/proximal/in')
    assert missing == 0 and printed == CASES['up_consistent_lg1']['stdout']


def test_synthetic_genome(gpu_ctx, tmp_path, capsys):
    """200 kbp in 7 contigs, 300 table sequences of window 53: a third from the reverse strand, 10 absent, 5 cut across a
    contig joint (they occur in the joined text only with the joining byte inside, so they must be reported missing)"""
    rng = np.random.default_rng(2026)
    nt = np.frombuffer(b'ACGT', dtype=np.uint8)
    lengths = [60000, 45000, 40000, 30000, 20000, 4950, 50]
    assert sum(lengths) == 200000
    contigs = [nt[rng.integers(0, 4, n)].tobytes().decode() for n in lengths]
    window, seqs, expect_missing = 53, [], []
    for i in range(285):
        c = contigs[int(rng.integers(0, 5))]
        s = int(rng.integers(0, len(c) - window + 1))
        seq = c[s:s + window]
        seqs.append(pg.reverse_complement(seq) if i % 3 == 0 else seq)
    for i in range(10):
        seqs.append(nt[rng.integers(0, 4, window)].tobytes().decode())
    for i in range(5):
        seqs.append(contigs[i][-(20 + i):] + contigs[i + 1][:window - 20 - i])
    with open(tmp_path / 'syn.fna', 'w') as f:
        for i, c in enumerate(contigs):
            f.write('>c%d\n' % i + '\n'.join(c[j:j + 80] for j in range(0, len(c), 80)) + '\n')
    labels = ['S_C%dU0' % i for i in range(len(seqs))]
    with open(tmp_path / 'nr.fna', 'w') as f:
        for label, seq in zip(labels, seqs):
            f.write('>%s\n%s\n' % (label, seq))
    cells = [(i, 0) for i in range(len(seqs))]
    want = model.validate_direct(labels, ['syn'], cells, [str(tmp_path / 'syn.fna')], str(tmp_path / 'nr.fna'), (-50, 3),
                                 'upstream')
    assert want.count('\tMissing') == 15                                 # (the 10 random ones and the 5 across a joint)
    case = {'index': labels, 'columns': ['syn'], 'cells': cells}
    capsys.readouterr()
    missing = pg.validate_upstream_table_direct(model.case_lsdf(case), [str(tmp_path / 'syn.fna')], str(tmp_path / 'nr.fna'),
                                                ctx=gpu_ctx)
    assert capsys.readouterr().out == want and missing == 15
