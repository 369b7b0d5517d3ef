"""pgx_sw_pairs / pgx_sw_pairs_dev (csrc/sw.hip) against the host model ncbi.host_sw, value for value: the lengths around
the kernel's strip, batches of more than one workgroup, the min_score gate, the length limit with closed-form answers, and the
device-pointer entry on caller tensors and a caller stream. host_sw itself is checked against a traceback in
tests/test_ncbi_host.py. The model computes some 2 million cells in this file, once per session."""
import numpy as np
import pytest

from pangenomix_amd import _native, ncbi

pytestmark = pytest.mark.gpu

AA20 = np.frombuffer(b'ACDEFGHIKLMNPQRSTVWY', dtype=np.uint8)
ACGT = np.frombuffer(b'ACGT', dtype=np.uint8)


def strip_width():
    return int(_native.lib().pgx_sw_strip_width())


def max_length():
    return int(_native.lib().pgx_sw_max_length())


def pack(seqs):
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return np.frombuffer(b''.join(bytes(s) for s in seqs), dtype=np.uint8), off


def model(seqs1, seqs2, pair_a, pair_b, min_score):
    out = np.zeros((len(pair_a), 8), dtype=np.int32)
    for p, (a, b) in enumerate(zip(pair_a, pair_b)):
        r = ncbi.host_sw(seqs1[a], seqs2[b], stats=True)
        if not (r[0] > 0 and r[0] >= min_score[p]):
            r[[1, 3, 5, 6, 7]] = 0
        out[p] = r
    return out


def relatives(rng, letters, lengths):
    """Per length one window of a common ancestor, and one mutated copy of another window of it (a tenth substituted, a
    block deleted from the longer ones): alignments with gaps that cross strips."""
    ancestor = letters[rng.integers(0, letters.size, 420)]
    plain, mutated = [], []
    for n in lengths:
        at = int(rng.integers(0, 40))
        plain.append(ancestor[at:at + n].tobytes())
        at = int(rng.integers(0, 40))
        s = ancestor[at:at + n + 7].copy()
        hit = rng.random(s.size) < 0.1
        s[hit] = letters[rng.integers(0, letters.size, int(hit.sum()))]
        if n > 20:
            cut = int(rng.integers(5, n - 10))
            s = np.concatenate([s[:cut], s[cut + 7:]])
        mutated.append(s[:n].tobytes())
    return plain, mutated


@pytest.fixture(scope='module')
def edge_sets():
    """{alphabet: (seqs1, seqs2, pair_a, pair_b, expected)}: the lengths 1, 2, W-1, W, W+1, 2W+1 and 333 crossed with
    each other."""
    w = strip_width()
    lengths = [1, 2, w - 1, w, w + 1, 2 * w + 1, 333]
    sets = {}
    for name, letters, seed in (('aa20', AA20, 1), ('acgt', ACGT, 2)):
        s1, s2 = relatives(np.random.default_rng(seed), letters, lengths)
        pa, pb = [x.ravel() for x in np.meshgrid(np.arange(len(lengths)), np.arange(len(lengths)), indexing='ij')]
        sets[name] = (s1, s2, pa, pb, model(s1, s2, pa, pb, np.ones(pa.size, dtype=np.int32)))
    return sets


@pytest.fixture(scope='module')
def batch():
    """150 pairs of mixed lengths over 60 + 40 sequences, more than one workgroup's sixteen; sequence 0 of set 2 is in 40 of
    them."""
    rng = np.random.default_rng(3)
    lengths = rng.integers(1, 121, 60).tolist()
    s1, s2 = relatives(rng, ACGT, lengths)
    s2 = s2[:40]
    pa = rng.integers(0, 60, 150)
    pb = rng.integers(0, 40, 150)
    pb[::3][:45] = 0
    ones = np.ones(150, dtype=np.int32)
    return s1, s2, pa, pb, model(s1, s2, pa, pb, ones)


def run(ctx, seqs1, seqs2, pair_a, pair_b, min_score):
    r1, o1 = pack(seqs1)
    r2, o2 = pack(seqs2)
    return ctx.sw_pairs(r1, o1, r2, o2, pair_a, pair_b, min_score)


@pytest.mark.parametrize('alphabet', ['aa20', 'acgt'])
def test_lengths_around_the_strip(gpu_ctx, edge_sets, alphabet):
    s1, s2, pa, pb, expected = edge_sets[alphabet]
    assert expected[:, 0].max() > 300 and (expected[:, 7] > 0).any()          # real alignments, some with gaps
    got = run(gpu_ctx, s1, s2, pa, pb, 1)
    np.testing.assert_array_equal(got, expected)


def test_no_pairs_and_one_pair(gpu_ctx, edge_sets):
    s1, s2, pa, pb, expected = edge_sets['aa20']
    assert run(gpu_ctx, s1, s2, pa[:0], pb[:0], 1).shape == (0, 8)
    last = pa.size - 1
    np.testing.assert_array_equal(run(gpu_ctx, s1, s2, pa[last:], pb[last:], 1), expected[last:])


def test_a_batch_of_several_workgroups(gpu_ctx, batch):
    s1, s2, pa, pb, expected = batch
    assert (pb == 0).sum() >= 40 and len(pa) > 16 * 4
    np.testing.assert_array_equal(run(gpu_ctx, s1, s2, pa, pb, 1), expected)


def test_min_score_gates_the_statistics(gpu_ctx, batch):
    s1, s2, pa, pb, expected = batch
    positive = np.flatnonzero(expected[:, 0] > 0)
    assert positive.size > 50
    at, below = positive[::2], positive[1::2]
    min_score = np.ones(pa.size, dtype=np.int32)
    min_score[at] = expected[at, 0]                        # exactly at the threshold: statistics
    min_score[below] = expected[below, 0] + 1              # one below it: the score and the end, zeros elsewhere
    got = run(gpu_ctx, s1, s2, pa, pb, min_score)
    np.testing.assert_array_equal(got[at], expected[at])
    want = expected[below].copy()
    want[:, [1, 3, 5, 6, 7]] = 0
    np.testing.assert_array_equal(got[below], want)
    assert (expected[below][:, 6] > 0).all()
    assert gpu_ctx.sw_last_stats_pairs() == pa.size - below.size - (expected[:, 0] == 0).sum()


def test_the_length_limit_in_closed_form(gpu_ctx):
    """W against W scores 11, W against A -3. A 16-bit score, position or count would wrap here (45,056 > 2^15)."""
    n = max_length()
    assert n >= 4096
    whole = b'W' * n
    half = (n - 10) // 2
    gapped = b'W' * half + b'A' * 10 + b'W' * (n - 10 - half)
    got = run(gpu_ctx, [whole], [whole, gapped], [0, 0], [0, 1], 1)
    assert got[0].tolist() == [11 * n, 0, n - 1, 0, n - 1, n, n, 0]
    # skipping the ten A costs 11 + 10 = 21, aligning them with W costs 30: one gap, and the first cell that holds the
    # n - 10 matches is query position n - 11 at the subject's end
    assert got[1].tolist() == [11 * (n - 10) - 21, 0, n - 11, 0, n - 1, n - 10, n, 1]


def test_one_residue_over_the_limit_is_refused(gpu_ctx):
    n = max_length()
    with pytest.raises(_native.PgxError, match='longer than pgx_sw_max_length'):
        run(gpu_ctx, [b'W' * (n + 1)], [b'W' * 8], [0], [0], 1)
    with pytest.raises(_native.PgxError, match='longer than pgx_sw_max_length'):
        run(gpu_ctx, [b'W' * 8], [b'W' * 8, b'W' * (n + 1)], [0, 0], [0, 1], 1)
    with pytest.raises(_native.PgxError, match='does not exist'):
        run(gpu_ctx, [b'W' * 8], [b'W' * 8], [1], [0], 1)


def test_two_calls_give_the_same_bytes(gpu_ctx, batch):
    s1, s2, pa, pb, _ = batch
    assert run(gpu_ctx, s1, s2, pa, pb, 1).tobytes() == run(gpu_ctx, s1, s2, pa, pb, 1).tobytes()


def test_other_bytes_and_lower_case(gpu_ctx):
    """a-z are the letters A-Z; every other byte is one more letter of class 20."""
    s1, s2 = [b'mkvlaagiww*ACDEF', b'MKVLAAGIWW'], [b'MKVLAAGIWW-ACDEF', b'mkvlaXgiww']
    pa, pb = [0, 1, 0], [0, 1, 1]
    np.testing.assert_array_equal(run(gpu_ctx, s1, s2, pa, pb, 1), model(s1, s2, pa, pb, [1, 1, 1]))


@pytest.mark.parametrize('stream_kind', ['null', 'side'])
def test_device_pointers_on_caller_tensors_and_streams(gpu_ctx, batch, stream_kind):
    import dev_entry_checks as dev
    s1, s2, pa, pb, expected = batch
    r1, o1 = pack(s1)
    r2, o2 = pack(s2)
    max_len = max(max(len(s) for s in s1), max(len(s) for s in s2))
    min_score = np.ones(pa.size, dtype=np.int32)
    min_score[::3] = 1 << 20
    want = gpu_ctx.sw_pairs(r1, o1, r2, o2, pa, pb, min_score)
    np.testing.assert_array_equal(want[1::3], expected[1::3])
    ws_bytes = gpu_ctx.sw_workspace_bytes(pa.size, max_len)
    assert ws_bytes > 0 and gpu_ctx.sw_workspace_bytes(pa.size, max_length() + 1) == 0
    results = []
    for fill in dev.FILLS:
        with dev.stream_scope(stream_kind) as stream:
            ins = [dev.upload(x) for x in (r1, o1, r2, o2, pa.astype(np.uint32), pb.astype(np.uint32), min_score)]
            out, ws = dev.guarded(pa.size * 32, fill), dev.guarded(ws_bytes, fill)
            with dev.unchanged(*ins):
                gpu_ctx.sw_pairs_dev(ins[0].ptr, ins[1].ptr, len(s1), ins[2].ptr, ins[3].ptr, len(s2), ins[4].ptr, ins[5].ptr,
                                     pa.size, ins[6].ptr, max_len, out.ptr, ws.ptr, ws_bytes, stream=stream)
        out.assert_guards_intact()
        ws.assert_guards_intact()
        results.append((out.numpy(np.int32).reshape(-1, 8),))
    np.testing.assert_array_equal(dev.same_bytes(results)[0], want)
    # a sequence longer than the promised max_len is skipped by the kernels and the call fails
    with dev.stream_scope('null') as stream:
        ins = [dev.upload(x) for x in (r1, o1, r2, o2, pa.astype(np.uint32), pb.astype(np.uint32), min_score)]
        out, ws = dev.guarded(pa.size * 32, 0xFF), dev.guarded(ws_bytes, 0xFF)
        with pytest.raises(_native.PgxError, match='longer than max_len'):
            gpu_ctx.sw_pairs_dev(ins[0].ptr, ins[1].ptr, len(s1), ins[2].ptr, ins[3].ptr, len(s2), ins[4].ptr, ins[5].ptr,
                                 pa.size, ins[6].ptr, max_len - 1, out.ptr, ws.ptr, ws_bytes, stream=stream)
    out.assert_guards_intact()
    ws.assert_guards_intact()
