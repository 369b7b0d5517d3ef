"""The exact dictionary match and the per-genome set difference on the device (csrc/dict.hip; include/pgx.h "Exact look-up of
whole byte strings", "Two sets of rows per genome") against the Python-dict and numpy-sets models
(tests/dict_match_model.py), and the four validators of pangenomix_amd.pangenome built on them against what the reference
printed and raised (tests/golden/table_fasta). Bytes and integers: every comparison is exact.
Everything runs twice, the second time with PGX_DICT_NARROW_HASH: 3 bits of hash, every probe collides, same output; those
runs are capped at 2,000 keys, the probe walk being quadratic there by design."""
import numpy as np
import pytest

import dev_entry_checks as dev
import dict_match_model as model
from pangenomix_amd import _native, pangenome as pg

pytestmark = pytest.mark.gpu

NARROW = 1                                   # PGX_DICT_NARROW_HASH
FLAGS = (0, NARROW)
NARROW_MAX_KEYS = 2000
CASES = model.load_cases()
TABLES = [(name, table) for name in sorted(CASES) for table in ('frame', 'lsdf') if table == 'frame' or model.is_binary(CASES[name])]


def step():
    return int(_native.lib().pgx_dict_group_bytes())


def random_bytes(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def check(ctx, keys, queries, flags, lead=0, query_lead=0):
    """dict_load + dict_query against the model; returns (first, last)"""
    assert not (flags & NARROW) or len(keys) <= NARROW_MAX_KEYS
    want_first, want_last = model.first_last(keys, queries)
    first = ctx.dict_load(*model.blob(keys, lead), flags=flags)
    last = ctx.dict_query(*model.blob(queries, query_lead))
    assert first.dtype == np.int32 and last.dtype == np.int32
    assert np.array_equal(first, want_first), 'first differs at %r' % np.flatnonzero(first != want_first)[:10].tolist()
    assert np.array_equal(last, want_last), 'last differs at %r' % np.flatnonzero(last != want_last)[:10].tolist()
    return first, last


def near_misses(key):
    """strings that differ from key in one byte -- the first, the last, one at each side of every chunk and group-step
    boundary -- or only in length"""
    out, S = [], step()
    at = {0, len(key) - 1}
    for b in list(range(16, len(key), 16))[:6] + list(range(S, len(key), S)):
        at.update((b - 1, b))
    for i in sorted(x for x in at if 0 <= x < len(key)):
        out.append(key[:i] + bytes([key[i] ^ 0x01]) + key[i + 1:])
    out += [key[:-1], key + b'\x00', key + key[-1:]] if key else [b'\x00']
    return out


@pytest.mark.parametrize('flags', FLAGS)
def test_lengths(flags, gpu_ctx):
    S = step()
    assert S % 16 == 0 and S >= 16
    rng = np.random.default_rng(1)
    lengths = sorted({0, 1, 15, 16, 17, S - 1, S, S + 1, 2 * S + 1, 4097}) + [40000]
    keys = [random_bytes(rng, n) for n in lengths]
    queries = list(keys)
    for key in keys:
        queries += near_misses(key)
    first, last = check(gpu_ctx, keys, queries, flags)
    assert first.tolist() == list(range(len(keys))) and last[:len(keys)].tolist() == list(range(len(keys)))
    assert (last[len(keys):] == -1).sum() >= len(queries) - len(keys) - 3       # (a near miss of '' or of 1 byte may be a key)
    # and with every near miss a key: keys that differ in one byte or in length only are told apart
    keys2 = list(dict.fromkeys(queries))
    first, last = check(gpu_ctx, keys2, queries + [k + b'\x01\x02' for k in keys], flags)
    assert first.tolist() == list(range(len(keys2))) and (last[:len(queries)] >= 0).all() and (last[len(queries):] == -1).all()


@pytest.mark.parametrize('flags', FLAGS)
def test_prefixes_of_each_other(flags, gpu_ctx):
    """only the length differs; every length from 0 past two group steps"""
    S = step()
    base = random_bytes(np.random.default_rng(2), 2 * S + 40)
    keys = [base[:n] for n in range(0, len(base) + 1, 3)]
    queries = [base[:n] for n in range(len(base) + 1)]
    first, last = check(gpu_ctx, keys, queries, flags)
    assert (last >= 0).sum() == len(keys)
    zeros = [b'\x00' * n for n in range(0, 70)]                                  # zero padding of the last chunk is no match
    check(gpu_ctx, zeros[::2], zeros, flags)


@pytest.mark.parametrize('flags', FLAGS)
def test_byte_values(flags, gpu_ctx):
    rng = np.random.default_rng(3)
    alphabet = np.array([0x00, 0x7f, 0x80, 0xff], dtype=np.uint8)
    keys = [alphabet[rng.integers(0, 4, int(n))].tobytes() for n in rng.integers(0, 40, 300)]
    keys += [bytes([v]) * n for v in (0x00, 0x7f, 0x80, 0xff) for n in (1, 16, 17, 33)]
    queries = keys[::2] + [alphabet[rng.integers(0, 4, int(n))].tobytes() for n in rng.integers(0, 6, 300)]
    queries += [bytes([v ^ 0x80]) * n for v in (0x00, 0x7f) for n in (1, 16, 17, 33)]
    first, last = check(gpu_ctx, keys, queries, flags)
    assert (last == -1).any() and (last >= 0).any() and (first != np.arange(len(keys))).any()


@pytest.mark.parametrize('flags', FLAGS)
@pytest.mark.parametrize('n_keys', (0, 1, 2, 63, 64, 65, 1000, 20000))
def test_key_counts(n_keys, flags, gpu_ctx):
    """20000 keys are past anything a table in LDS alone would hold; about half the queries are absent"""
    if flags & NARROW and n_keys > NARROW_MAX_KEYS:
        n_keys = NARROW_MAX_KEYS
    rng = np.random.default_rng(n_keys)
    lengths = rng.integers(0, 80, n_keys)
    keys = [random_bytes(rng, int(n)) for n in lengths]
    n_queries = max(n_keys, 40)
    queries = []
    for i in range(n_queries):
        if n_keys and rng.random() < 0.5:
            queries.append(keys[int(rng.integers(0, n_keys))])
        else:
            queries.append(random_bytes(rng, int(rng.integers(3, 80))))
    first, last = check(gpu_ctx, keys, queries, flags)
    if n_keys == 0:
        assert (last == -1).all()
    elif n_keys >= 63:
        assert 0 < (last == -1).sum() < n_queries


@pytest.mark.parametrize('flags', FLAGS)
def test_equal_keys(flags, gpu_ctx):
    rng = np.random.default_rng(4)
    a, b, c = random_bytes(rng, 300), random_bytes(rng, 21), b''
    keys = [random_bytes(rng, int(n)) for n in rng.integers(1, 50, 500)]
    for at in (5, 390):
        keys[at] = a                                                             # twice
    hundred = list(range(7, 500, 4))[:100]
    for at in hundred:
        keys[at] = b                                                             # 100 times
    keys[3] = keys[200] = c
    first, last = check(gpu_ctx, keys, [a, b, c, a[:-1]], flags)
    assert first[390] == 5 and first[5] == 5 and last.tolist() == [390, hundred[-1], 200, -1]
    assert len(hundred) == 100 and (first == 7).sum() == 100
    for same in (a, b'\x80' * 17, b''):                                          # all keys equal; all strings empty
        first, last = check(gpu_ctx, [same] * 130, [same, same + b'\x00', same[:-1] if same else b'\x00'], flags)
        assert (first == 0).all() and last.tolist() == [129, -1, -1]


@pytest.mark.parametrize('flags', FLAGS)
def test_offsets_that_do_not_start_at_zero(flags, gpu_ctx):
    rng = np.random.default_rng(5)
    S = step()
    keys = [random_bytes(rng, int(n)) for n in list(rng.integers(0, 3 * S, 60)) + [0, 16, S, 5]]
    queries = keys[::-1] + [k + b'x' for k in keys[:10]]
    for lead in range(1, 16):
        check(gpu_ctx, keys, queries, flags, lead=lead, query_lead=16 - lead)


def test_reuse_of_a_loaded_set(gpu_ctx):
    rng = np.random.default_rng(6)
    keys = [random_bytes(rng, int(n)) for n in rng.integers(0, 300, 500)]
    other = [random_bytes(rng, int(n)) for n in rng.integers(0, 30, 70)] + keys[:5]
    q1, q2 = keys[:50] + other[:20], other + keys[100:120]
    gpu_ctx.dict_load(*model.blob(keys))
    for _ in range(2):                                                           # dict_query twice on one load
        assert np.array_equal(gpu_ctx.dict_query(*model.blob(q1)), model.first_last(keys, q1)[1])
    assert np.array_equal(gpu_ctx.dict_query(*model.blob(q2)), model.first_last(keys, q2)[1])
    assert gpu_ctx.dict_load(*model.blob(other), want_first=False) is None       # a second load replaces the first
    assert np.array_equal(gpu_ctx.dict_query(*model.blob(q1)), model.first_last(other, q1)[1])
    assert np.array_equal(gpu_ctx.dict_query(*model.blob(q2)), model.first_last(other, q2)[1])
    assert gpu_ctx.dict_query(*model.blob([])).shape == (0,)
    gpu_ctx.dict_load(*model.blob([]))
    assert gpu_ctx.dict_query(*model.blob(q1)).tolist() == [-1] * len(q1)


# -- sets diff -------------------------------------------------------------------------------------------------------------
def coo_case(rng, n_rows, n_genomes, kind):
    dense_a = rng.random((n_rows, n_genomes)) < 0.4
    dense_b = dense_a ^ (rng.random((n_rows, n_genomes)) < 0.1)
    if kind == 'empty_a':
        dense_a[:] = False
    elif kind == 'empty_b':
        dense_b[:] = False
    elif kind == 'equal':
        dense_b = dense_a.copy()
    a, b = np.nonzero(dense_a), np.nonzero(dense_b)
    if kind == 'duplicates':
        a = tuple(np.concatenate([x, x[::3], x[:5]]) for x in a)
        b = tuple(np.concatenate([x[::2], x]) for x in b)
    return a[0].astype(np.int32), a[1].astype(np.int32), b[0].astype(np.int32), b[1].astype(np.int32)


@pytest.mark.parametrize('n_genomes', (1, 2, 65))
@pytest.mark.parametrize('n_rows', (1, 63, 64, 65, 4097))
def test_sets_diff(n_rows, n_genomes, gpu_ctx):
    rng = np.random.default_rng(n_rows * 100 + n_genomes)
    for kind in ('random', 'empty_a', 'empty_b', 'equal', 'duplicates'):
        args = coo_case(rng, n_rows, n_genomes, kind)
        want = model.sets_diff(*args, n_rows, n_genomes)
        got = gpu_ctx.genome_sets_diff(*args, n_rows, n_genomes)
        assert got[0].dtype == np.uint32 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), kind
        if kind == 'equal':
            assert not got[0].any() and not got[1].any()
    assert all(x.shape == (0,) for x in gpu_ctx.genome_sets_diff([], [], [], [], 5, 0))
    with pytest.raises(_native.PgxError) as e:                                   # a row out of range
        gpu_ctx.genome_sets_diff([n_rows], [0], [], [], n_rows, n_genomes)
    assert e.value.status == -1


@pytest.mark.parametrize('stream', dev.STREAMS)
def test_sets_diff_device_entry_never_counts_pad_bits(stream, gpu_ctx):
    lib = _native.lib()
    for n_rows, n_genomes in ((1, 2), (63, 1), (64, 3), (65, 65), (4097, 2)):
        rng = np.random.default_rng(n_rows)
        stride = int(lib.pgx_bitmap_stride_words(n_rows))
        # garbage everywhere, pad bits and pad words included: only bits below n_rows count
        a = rng.integers(0, 1 << 63, (n_genomes, stride), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
        b = rng.integers(0, 1 << 63, (n_genomes, stride), dtype=np.uint64) * np.uint64(2)
        unpack = lambda bits: ((bits[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool) \
            .reshape(n_genomes, -1)[:, :n_rows]                                  # noqa: E731
        da, db = unpack(a), unpack(b)
        per_fill = []
        for fill in dev.FILLS:
            with dev.stream_scope(stream) as handle:
                d_a, d_b = dev.upload(a), dev.upload(b)
                out_a, out_b = dev.guarded(4 * n_genomes, fill), dev.guarded(4 * n_genomes, fill)
                with dev.unchanged(d_a, d_b):
                    gpu_ctx.genome_sets_diff_dev(d_a.ptr, d_b.ptr, n_rows, n_genomes, out_a.ptr, out_b.ptr, handle)
            out_a.assert_guards_intact()
            out_b.assert_guards_intact()
            got = out_a.numpy(np.uint32), out_b.numpy(np.uint32)
            assert np.array_equal(got[0], (da & ~db).sum(axis=1)) and np.array_equal(got[1], (db & ~da).sum(axis=1))
            per_fill.append(got)
        dev.same_bytes(per_fill)
    out = dev.guarded(8, 0x5A)
    with pytest.raises(_native.PgxError):
        gpu_ctx.genome_sets_diff_dev(out.ptr, out.ptr, 1 << 31, 1, out.ptr, out.ptr)
    assert out.is_still_garbage()
    dev.assert_no_allocation(lambda: gpu_ctx.genome_sets_diff_dev(d_a.ptr, d_b.ptr, n_rows, n_genomes, out_a.ptr, out_b.ptr))


# -- the device entry ------------------------------------------------------------------------------------------------------
def dev_case(seed, n_keys=300):
    rng = np.random.default_rng(seed)
    S = step()
    keys = [random_bytes(rng, int(n)) for n in rng.integers(0, 2 * S + 20, n_keys)]
    for at in range(3, n_keys, 17):
        keys[at] = keys[at // 2]
    queries = keys[::3] + [random_bytes(rng, int(n)) for n in rng.integers(0, 40, 100)] + [k[:-1] for k in keys[:40] if k]
    return keys, queries


def run_dev(ctx, keys, queries, flags, fill, stream, want_first=True, lead=0):
    kb, ko = model.blob(keys, lead)
    qb, qo = model.blob(queries, lead)
    ws_bytes = _native.lib().pgx_dict_workspace_bytes(kb.size, len(keys))
    assert ws_bytes > 0
    with dev.stream_scope(stream) as handle:
        d_kb, d_ko, d_qb, d_qo = dev.upload(kb), dev.upload(ko), dev.upload(qb), dev.upload(qo)
        first, last, ws = dev.guarded(4 * len(keys), fill), dev.guarded(4 * len(queries), fill), dev.guarded(ws_bytes, fill)
        with dev.unchanged(d_kb, d_ko, d_qb, d_qo):
            ctx.dict_match_dev(d_kb.ptr, d_ko.ptr, len(keys), d_qb.ptr, d_qo.ptr, len(queries), first.ptr if want_first else None,
                               last.ptr, ws.ptr, ws_bytes, flags, handle)
    for buf in (first, last, ws):
        buf.assert_guards_intact()
    assert want_first or first.is_still_garbage()
    return first.numpy(np.int32), last.numpy(np.int32)


@pytest.mark.parametrize('flags', FLAGS)
@pytest.mark.parametrize('stream', dev.STREAMS)
def test_device_entry_on_caller_tensors(stream, flags, gpu_ctx):
    for seed, n_keys in ((1, 300), (2, 1), (3, 65)):
        keys, queries = dev_case(seed, n_keys)
        want = model.first_last(keys, queries)
        per_fill = []
        for fill in dev.FILLS:                                        # outputs and the workspace pre-filled with garbage
            got = run_dev(gpu_ctx, keys, queries, flags, fill, stream)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            per_fill.append(got)
        dev.same_bytes(per_fill)
    keys, queries = dev_case(4)
    _, last = run_dev(gpu_ctx, keys, queries, flags, 0xFF, stream, want_first=False, lead=7)
    assert np.array_equal(last, model.first_last(keys, queries)[1])


@pytest.mark.parametrize('flags', FLAGS)
def test_device_entry_blobs_that_are_not_16_byte_aligned(flags, gpu_ctx):
    """base pointers off by 1 (and more) from 16-byte alignment: wide loads only where aligned words lie inside the blob"""
    import torch
    keys, queries = dev_case(5)
    keys += [b'', b'Z']
    queries = [b'Z', b''] + queries + [b'Z']                         # strings on the blob's very first and last bytes
    want = model.first_last(keys, queries)
    (kb, ko), (qb, qo) = model.blob(keys), model.blob(queries)
    ws_bytes = _native.lib().pgx_dict_workspace_bytes(kb.size, len(keys))
    for shift in (1, 15, 8):
        bufs = []
        for data in (kb, qb):
            # the blob sits at the very end of its allocation's payload, a guard band behind it
            g = dev.guarded(shift + data.size, 0x5A)
            g.raw[dev.GUARD + shift:dev.GUARD + shift + data.size] = torch.from_numpy(data.copy()).cuda()
            bufs.append(g)
        d_ko, d_qo = dev.upload(ko), dev.upload(qo)
        first, last, ws = dev.guarded(4 * len(keys), 0xFF), dev.guarded(4 * len(queries), 0xFF), dev.guarded(ws_bytes, 0xFF)
        torch.cuda.synchronize()
        gpu_ctx.dict_match_dev(bufs[0].ptr + shift, d_ko.ptr, len(keys), bufs[1].ptr + shift, d_qo.ptr, len(queries), first.ptr,
                               last.ptr, ws.ptr, ws_bytes, flags)
        assert np.array_equal(first.numpy(np.int32), want[0]) and np.array_equal(last.numpy(np.int32), want[1])
        for buf in (first, last, ws):
            buf.assert_guards_intact()


def test_device_entry_does_not_allocate(gpu_ctx):
    keys, queries = dev_case(6)
    (kb, ko), (qb, qo) = model.blob(keys), model.blob(queries)
    ws_bytes = _native.lib().pgx_dict_workspace_bytes(kb.size, len(keys))
    d_kb, d_ko, d_qb, d_qo = dev.upload(kb), dev.upload(ko), dev.upload(qb), dev.upload(qo)
    first, last, ws = dev.guarded(4 * len(keys), 0xFF), dev.guarded(4 * len(queries), 0xFF), dev.guarded(ws_bytes, 0xFF)
    dev.assert_no_allocation(lambda: gpu_ctx.dict_match_dev(d_kb.ptr, d_ko.ptr, len(keys), d_qb.ptr, d_qo.ptr, len(queries),
                                                            first.ptr, last.ptr, ws.ptr, ws_bytes))


def test_invalid_calls_are_refused_before_anything_is_written():
    """on a context of its own: nothing is loaded yet"""
    lib = _native.lib()
    ctx = _native.Context(0)
    try:
        blob, off = model.blob([b'AC', b'GT', b'A'])
        out = np.full(3, 0x6E6E6E6E, dtype=np.int32)
        P = _native._ptr

        def refused(rc, who):
            assert rc == -1, who                                                 # PGX_ERR_INVALID
            assert (out == 0x6E6E6E6E).all(), who
        refused(lib.pgx_dict_query(ctx._h, P(blob), P(off), 3, P(out)), 'query before any load')
        assert 'loaded' in lib.pgx_last_error().decode()
        refused(lib.pgx_dict_load(ctx._h, P(blob), P(off), 1 << 24, 0, P(out)), 'n_keys')
        refused(lib.pgx_dict_load(ctx._h, P(blob), P(off), 3, 2, P(out)), 'flags')
        down = off.copy()
        down[2] = 1
        refused(lib.pgx_dict_load(ctx._h, P(blob), P(down), 3, 0, P(out)), 'decreasing offsets')
        big = off.copy()
        big[3] = 1 << 32
        refused(lib.pgx_dict_load(ctx._h, P(blob), P(big), 3, 0, P(out)), 'blob of 2^32 bytes')
        refused(lib.pgx_dict_query(ctx._h, P(blob), P(off), 3, P(out)), 'a refused load loads nothing')
        assert lib.pgx_dict_workspace_bytes(1 << 32, 3) == 0 and lib.pgx_dict_workspace_bytes(5, 1 << 24) == 0
        assert lib.pgx_dict_workspace_bytes(5, 3) == 64 * 8 and lib.pgx_dict_workspace_bytes(0, 0) > 0
        ctx.dict_load(blob, off)
        refused(lib.pgx_dict_query(ctx._h, P(blob), P(down), 3, P(out)), 'decreasing query offsets')
        refused(lib.pgx_dict_query(ctx._h, P(blob), P(big), 3, P(out)), 'query blob of 2^32 bytes')
        for n_queries in (1 << 31, (1 << 32) - 1):                               # (2^32 - 1: the round count would wrap)
            refused(lib.pgx_dict_query(ctx._h, P(blob), P(off), n_queries, P(out)), 'n_queries')
        assert ctx.dict_query(blob, off).tolist() == [0, 1, 2]                   # the loaded set is still there
        with pytest.raises(ValueError):
            ctx.dict_load(blob, off + np.uint64(1))
        # the device entry refuses the same without touching its buffers
        g = dev.guarded(4096, 0x5A)
        ws_bytes = lib.pgx_dict_workspace_bytes(5, 3)
        for n_keys, flags, ws in ((1 << 24, 0, 1 << 30), (3, 2, ws_bytes), (3, 0, ws_bytes - 8), (3, 0, 0)):
            with pytest.raises(_native.PgxError) as e:
                ctx.dict_match_dev(g.ptr, g.ptr, n_keys, g.ptr, g.ptr, 3, g.ptr, g.ptr, g.ptr, ws, flags)
            assert e.value.status == -1
        for n_queries in (1 << 31, (1 << 32) - 1):
            with pytest.raises(_native.PgxError) as e:
                ctx.dict_match_dev(g.ptr, g.ptr, 3, g.ptr, g.ptr, n_queries, g.ptr, g.ptr, g.ptr, ws_bytes)
            assert e.value.status == -1
        assert g.is_still_garbage()
        g.assert_guards_intact()
    finally:
        ctx.close()


# -- the validators --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('batch', (None, 1))
@pytest.mark.parametrize('name,table', TABLES)
def test_validators_equal_the_reference(name, table, batch, gpu_ctx, capsys, monkeypatch):
    """stdout (paths normalised), return value and exceptions, at both batch sizes, through the wrapper and directly"""
    case = CASES[name]
    if batch is not None:
        monkeypatch.setattr(pg, 'TABLE_FASTA_BATCH_BYTES', batch)
    wrapper = {'allele': pg.validate_allele_table, 'upstream': pg.validate_upstream_table,
               'downstream': pg.validate_downstream_table}[case['kind']]
    for fn in (wrapper, pg.validate_table_against_fasta):
        df = model.case_frame(case) if table == 'frame' else model.case_lsdf(case)
        printed, result, exc = model.run_validator(fn, case, df, capsys, ctx=gpu_ctx)
        model.assert_as_recorded(case, printed, result, exc)


def test_validator_on_the_table_the_builder_returns(gpu_ctx, golden_dir, tmp_path, capsys):
    """build_cds_pangenome's LSDF goes straight into validate_allele_table: every genome holds what the table records"""
    import os
    import shutil
    din = tmp_path / 'in'
    shutil.copytree(os.path.join(golden_dir, 'cds', 'in'), din)
    (tmp_path / 'out').mkdir()
    paths = sorted(str(p) for p in din.glob('*.faa'))
    df_alleles, _ = pg.build_cds_pangenome(paths, str(tmp_path / 'out'), name='T')
    capsys.readouterr()
    assert pg.validate_allele_table(df_alleles, paths, str(tmp_path / 'out' / 'T_nr.faa'), ctx=gpu_ctx) == 0
    printed = capsys.readouterr().out
    assert printed.count('Validating genome') == 6 and printed.endswith('Feature Table Inconsistencies: 0\n')


def test_synthetic_set_with_planted_differences(gpu_ctx, tmp_path, capsys):
    """40 genomes x 300 records over 2,000 non-redundant sequences with 50 repeated ones: the device against the SHA-256
    restatement"""
    rng = np.random.default_rng(2026)
    aa = np.frombuffer(b'ACDEFGHIKLMNPQRSTVWY', dtype=np.uint8)
    seqs = [aa[rng.integers(0, 20, int(n))].tobytes().decode() for n in rng.integers(20, 900, 2000)]
    for i in range(50):
        seqs[1900 + i] = seqs[i * 7]                                             # COLLISION: the later header wins
    labels = ['S_C%dA0' % i for i in range(2000)]
    with open(tmp_path / 'nr.faa', 'w') as f:
        for label, seq in zip(labels, seqs):
            f.write('>%s\n%s\n' % (label, '\n'.join(seq[j:j + 70] for j in range(0, len(seq), 70))))
    columns, paths, cells = ['s%02d' % g for g in range(40)], [], {}
    winner = {seq: i for i, seq in enumerate(seqs)}
    for g, column in enumerate(columns):
        picks = rng.choice(2000, 300, replace=False)
        path = str(tmp_path / (column + '.faa'))
        paths.append(path)
        with open(path, 'w') as f:
            for n, i in enumerate(picks.tolist()):
                f.write('>%s|%d\n%s\n' % (column, n, seqs[i]))
                cells[(winner[seqs[i]], g)] = 1
            if g % 9 == 0:
                f.write('>extra\nMKV%sLLL\n' % ('A' * g))                        # absent from the nr set: counts nowhere
        if g % 7 == 3:
            del cells[(winner[seqs[int(picks[0])]], g)]                          # genome only
        if g % 5 == 2:
            cells[(int(np.setdiff1d(np.arange(2000), [winner[seqs[i]] for i in picks])[g]), g)] = 1     # table only
    want = model.validate(labels, columns, cells, paths, str(tmp_path / 'nr.faa'))
    assert want.count('COLLISION') == 50 and want.count('Table only') == len({g for g in range(40) if g % 7 == 3 or g % 5 == 2})
    case = {'index': labels, 'columns': columns, 'cells': sorted(cells), 'other': []}
    capsys.readouterr()
    count = pg.validate_allele_table(model.case_lsdf(case), paths, str(tmp_path / 'nr.faa'), ctx=gpu_ctx)
    assert capsys.readouterr().out == want and count == want.count('Table only')
