"""pgx_sw_pairs / pgx_sw_pairs_dev (csrc/sw.hip) on the paths that the real workload takes on every call and that
tests/test_gpu_sw_pairs.py does not reach: more than two grid rounds of both passes (a lane group that starts a second pair
over its own stale workspace rows, and the skip of a slot past the end), a compaction with more than one slot per thread,
forced ties of the best cell across lanes, strips and 16-step blocks, one gap that crosses strip boundaries on purpose, late
starts at the length limit, and the device entry's refusals. Every row is compared exactly. The references are the model
ncbi.host_sw and, where the size allows it, the full-matrix traceback of tests/sw_reference.py, which shares nothing with
either; the closed forms are asserted on the CPU by the builders below (build_*), which need no GPU.

W = pgx_sw_strip_width(), R_score / R_stats = Context.sw_round_pairs(False / True) stay symbolic: the batch sizes follow the
device. On an MI355X (256 CUs) R_score = 32,768 and R_stats = 8,192, and the largest batch is 65,589 pairs of
281,584,282 cells (the sum of m x n over the seeded draw; the pool's mean pair has 4,260 cells).

CPU reference work of this file, once per session, as measured: the pool's 196 rows 1.3 s (0.8e6 cells), the ties 0.6 s
(0.2e6 cells, most of them in the traceback too), the strip-crossing gaps 1.0 s (1.2e6 cells), the limit pair and the long
relatives 2.0 s (17.7e6 cells), the two-letter relatives 0.2 s (0.09e6 cells of the traceback): 5.1 s."""
import time

import numpy as np
import pytest

import sw_reference as ref
from pangenomix_amd import _native, ncbi

pytestmark = pytest.mark.gpu

STATS_COLUMNS = [1, 3, 5, 6, 7]                 # what a pair below its min_score does not get
REFUSED = 'does not exist, offsets decrease, or a sequence is longer than max_len'


def strip_width():
    return int(_native.lib().pgx_sw_strip_width())


def max_length():
    return int(_native.lib().pgx_sw_max_length())


def model_row(q, s):
    return ncbi.host_sw(q, s).tolist()


def score_only_rows(rows):
    out = np.array(rows, dtype=np.int32)
    out[:, STATS_COLUMNS] = 0
    return out


# ---- builders: sequences and their expected rows, closed forms asserted against the references (CPU only) -----------------------
def build_pool(w):
    """14 sequences per side, windows of one ancestor over AA20 (set 2: a tenth substituted and a block of seven deleted
    from the longer ones, as test_gpu_sw_pairs.relatives), of the lengths below; rows[a * 14 + b] = host_sw(set1[a], set2[b])."""
    lengths = [0, 1, 15, 16, 17, w - 1, w, w + 1, w + 15, w + 16, 2 * w - 1, 2 * w, 2 * w + 1, 2 * w + 2]
    rng = np.random.default_rng(5)
    ancestor = ref.AA20[rng.integers(0, ref.AA20.size, 2 * w + 60)]
    set1, set2 = [], []
    for n in lengths:
        at = int(rng.integers(0, 40))
        set1.append(ancestor[at:at + n].tobytes())
        at = int(rng.integers(0, 40))
        s = ancestor[at:at + n + 7].copy()
        hit = rng.random(s.size) < 0.1
        s[hit] = ref.AA20[rng.integers(0, ref.AA20.size, int(hit.sum()))]
        if n > 20:
            cut = int(rng.integers(5, n - 10))
            s = np.concatenate([s[:cut], s[cut + 7:]])
        set2.append(s[:n].tobytes())
    assert [len(x) for x in set1] == lengths and [len(x) for x in set2] == lengths
    rows = np.array([model_row(q, s) for q in set1 for s in set2], dtype=np.int32)
    assert (rows[:, 7] > 0).any() and (rows[:, 0] > 0).sum() > 150
    return set1, set2, rows


def build_ties(w):
    """(queries, subjects, rows, S): per spacer length four pairs whose best score S is reached in two cells."""
    X = ref.core(30, 7)
    Y = np.random.default_rng(8).permutation(np.frombuffer(X, dtype=np.uint8)).tobytes()
    S = ref.self_score(X)
    assert X != Y and sorted(X) == sorted(Y) and ref.self_score(Y) == S
    assert ref.sub(b'W', b'P') < 0
    qs, ss, rows = [], [], []
    for sp in (1, 3, 4, 34, 60, w, 2 * w + 2):
        wq, ps = b'W' * sp, b'P' * sp
        first = [S, 0, 29, 0, 29, 30, 30, 0]
        crossed = [S, 0, 29, 30 + sp, 59 + sp, 30, 30, 0]
        for q, s, want in ((X + wq + X, X, first),                       # the smallest i wins
                           (X, X + ps + X, first),                       # the smallest j wins
                           (X + wq + Y, Y + ps + X, crossed),            # the smallest i beats the smaller j
                           (Y + wq + X, X + ps + Y, crossed)):
            assert model_row(q, s) == want, (sp, q, s)
            if sp <= w:
                assert ref.traceback_sw(q, s) == want, (sp, q, s)
            qs.append(q); ss.append(s); rows.append(want)
    return qs, ss, np.array(rows, dtype=np.int32), S


def build_strip_gaps(w):
    """(queries, subjects, rows): one gap of k residues after `at` matched ones, as an F gap (q holds the insert: the gap runs
    along the query, through strip boundaries) and with the sequences exchanged (an E gap, through 16-step blocks)."""
    qs, ss, rows = [], [], []
    for k in (1, 10, w, w + 6, 100):
        for at in (30, 60, w - 1, w):
            a, b = ref.core(at, 100 + at), ref.core(150 - at, 200 + at + k)
            q, s = a + b'W' * k + b, a + b
            score = ref.self_score(s) - (11 + k)
            for x, y, want in ((q, s, [score, 0, 149 + k, 0, 149, 150, 150 + k, 1]),
                               (s, q, [score, 0, 149, 0, 149 + k, 150, 150 + k, 1])):
                assert model_row(x, y) == want, (k, at)
                qs.append(x); ss.append(y); rows.append(want)
    return qs, ss, np.array(rows, dtype=np.int32)


def build_late_starts(n):
    """(queries, subjects, rows): a pair of the limit's length whose alignment starts past position 3,900 on both sides and
    holds one gap, and relatives of 1,000 x 900 with three planted indels (16 strips)."""
    rng = np.random.default_rng(9)
    c = ref.core(90, 10)
    q = ref.CORE_LETTERS[rng.integers(0, ref.CORE_LETTERS.size, n - 90)].tobytes() + c
    s = ref.CORE_LETTERS[rng.integers(0, ref.CORE_LETTERS.size, n - 100)].tobytes() + c[:40] + c[47:]
    s += b'P' * (n - len(s))
    assert len(q) == n and len(s) == n
    late = model_row(q, s)
    assert late[1] > 3900 and late[3] > 3900 and late[7] == 1, late
    base = ref.AA20[rng.integers(0, ref.AA20.size, 1000)]
    other = base.copy()
    hit = rng.random(other.size) < 0.1
    other[hit] = ref.AA20[rng.integers(0, ref.AA20.size, int(hit.sum()))]
    other = np.concatenate([other[:250], other[320:600], other[650:800], ref.AA20[rng.integers(0, ref.AA20.size, 20)], other[800:]])
    q2, s2 = base.tobytes(), other.tobytes()
    assert (len(q2), len(s2)) == (1000, 900)
    long_row = model_row(q2, s2)
    assert long_row[7] >= 2 and long_row[6] > 800, long_row
    return [q, q2], [s, s2], np.array([late, long_row], dtype=np.int32)


def build_two_letter():
    pairs = ref.two_letter_relatives()
    rows = [ref.traceback_sw(q, s) for q, s in pairs]
    assert len(pairs) >= 8 and all(r[7] > 0 for r in rows)
    assert all(len(q) > strip_width() for q, _ in pairs)
    return [q for q, _ in pairs], [s for _, s in pairs], np.array(rows, dtype=np.int32)


# ---- fixtures: each reference once per session of this file ------------------------------------------------------------------
@pytest.fixture(scope='module')
def pool():
    set1, set2, rows = build_pool(strip_width())
    rows.setflags(write=False)
    return set1, set2, rows


@pytest.fixture(scope='module')
def big_batch(gpu_ctx, pool):
    """(pair_a, pair_b, expected): more than two rounds of the score pass, the last round and its last workgroup partial."""
    r_score = gpu_ctx.sw_round_pairs(False)
    n_pairs = 2 * r_score + 3 * 16 + 5
    if n_pairs > 200000:
        pytest.skip('two rounds of the score pass are %d pairs on this device: too many for a quick test' % n_pairs)
    index = np.random.default_rng(6).integers(0, 196, n_pairs)
    assert np.unique(index).size == 196
    expected = pool[2][index]
    expected.setflags(write=False)
    return (index // 14).astype(np.uint32), (index % 14).astype(np.uint32), expected


@pytest.fixture(scope='module')
def ties():
    return build_ties(strip_width())


@pytest.fixture(scope='module')
def strip_gaps():
    return build_strip_gaps(strip_width())


@pytest.fixture(scope='module')
def late_starts():
    return build_late_starts(max_length())


@pytest.fixture(scope='module')
def two_letter():
    return build_two_letter()


# ---- running --------------------------------------------------------------------------------------------------------------------
def report(name, ctx, n_pairs, seconds):
    print('sw_rounds %s: n_pairs=%d stats_pairs=%d wall=%.3fs R_score=%d R_stats=%d'
          % (name, n_pairs, ctx.sw_last_stats_pairs(), seconds, ctx.sw_round_pairs(False), ctx.sw_round_pairs(True)))


def run_host(ctx, name, set1, set2, pair_a, pair_b, min_score):
    r1, o1 = ref.pack(set1)
    r2, o2 = ref.pack(set2)
    t0 = time.perf_counter()
    got = ctx.sw_pairs(r1, o1, r2, o2, pair_a, pair_b, min_score)
    report(name, ctx, len(pair_a), time.perf_counter() - t0)
    return got


def run_one_to_one(ctx, name, queries, subjects, min_score=1):
    both = np.arange(len(queries))
    return run_host(ctx, name, queries, subjects, both, both, min_score)


def run_dev(ctx, name, arrays, n1, n2, max_len, fill, stream_kind='null'):
    """pgx_sw_pairs_dev on fresh uploads of arrays = (res1, off1, res2, off2, pair_a, pair_b, min_score) and on an out and
    a workspace between guard bands, filled with `fill`: (rows, the PgxError or None). Guards and inputs are checked."""
    import dev_entry_checks as dev
    n_pairs = arrays[4].size
    ws_bytes = ctx.sw_workspace_bytes(n_pairs, max_len)
    assert ws_bytes > 0
    error = None
    with dev.stream_scope(stream_kind) as stream:
        ins = [dev.upload(x) for x in arrays]
        out, ws = dev.guarded(n_pairs * 32, fill), dev.guarded(ws_bytes, fill)
        with dev.unchanged(*ins):
            t0 = time.perf_counter()
            try:
                ctx.sw_pairs_dev(ins[0].ptr, ins[1].ptr, n1, ins[2].ptr, ins[3].ptr, n2, ins[4].ptr, ins[5].ptr, n_pairs,
                                 ins[6].ptr, max_len, out.ptr, ws.ptr, ws_bytes, stream=stream)
            except _native.PgxError as e:
                error = e
            report(name, ctx, n_pairs, time.perf_counter() - t0)
    out.assert_guards_intact()
    ws.assert_guards_intact()
    return out.numpy(np.int32).reshape(-1, 8), error


def dev_arrays(set1, set2, pair_a, pair_b, min_score):
    r1, o1 = ref.pack(set1)
    r2, o2 = ref.pack(set2)
    pair_a = np.ascontiguousarray(pair_a, dtype=np.uint32)
    return [r1, o1, r2, o2, pair_a, np.ascontiguousarray(pair_b, dtype=np.uint32),
            np.ascontiguousarray(np.broadcast_to(np.asarray(min_score, dtype=np.int32), pair_a.shape))]


# ---- C1, C2: more than two rounds of both passes --------------------------------------------------------------------------------
def test_more_than_two_rounds_of_both_passes(gpu_ctx, pool, big_batch):
    set1, set2, _ = pool
    pair_a, pair_b, expected = big_batch
    r_score, r_stats = gpu_ctx.sw_round_pairs(False), gpu_ctx.sw_round_pairs(True)
    assert r_score > 0 and r_score % 16 == 0 and r_stats > 0 and r_stats % 16 == 0
    assert 2 * r_score < pair_a.size < 3 * r_score and pair_a.size % 16 != 0
    got = run_host(gpu_ctx, 'rounds_host', set1, set2, pair_a, pair_b, 1)
    positive = int((expected[:, 0] > 0).sum())
    print('sw_rounds rounds_host: positive expected scores %d' % positive)
    assert positive > 2 * r_stats
    assert gpu_ctx.sw_last_stats_pairs() == positive
    np.testing.assert_array_equal(got, expected)
    empty = (pair_a == 0) | (pair_b == 0)                                        # sequence 0 of either side has no residues
    assert empty.sum() > 1000 and not got[empty].any()


def test_the_same_rounds_in_the_callers_order_on_device_memory(gpu_ctx, pool, big_batch):
    """The host entry hands a lane group ever shorter pairs; here a short pair is followed by a long one over the short
    one's workspace rows."""
    import dev_entry_checks as dev
    set1, set2, _ = pool
    pair_a, pair_b, expected = big_batch
    arrays = dev_arrays(set1, set2, pair_a, pair_b, 1)
    max_len = max(len(x) for x in set1 + set2)
    results = []
    for fill, stream_kind in zip(dev.FILLS, dev.STREAMS):
        got, error = run_dev(gpu_ctx, 'rounds_dev_fill_%02x' % fill, arrays, len(set1), len(set2), max_len, fill, stream_kind)
        assert error is None
        assert gpu_ctx.sw_last_stats_pairs() == (expected[:, 0] > 0).sum()
        results.append((got,))
    # one more residue per workspace row: every lane group's rows lie elsewhere
    got, error = run_dev(gpu_ctx, 'rounds_dev_stride', arrays, len(set1), len(set2), max_len + 1, dev.FILLS[0])
    assert error is None
    results.append((got,))
    np.testing.assert_array_equal(dev.same_bytes(results)[0], expected)


# ---- C3: the compaction past one slot per thread --------------------------------------------------------------------------------
def passing(pattern, n):
    mask = np.zeros(n, dtype=bool)
    if pattern == 'all':
        mask[:] = True
    elif pattern == 'first':
        mask[0] = True
    elif pattern == 'last':
        mask[n - 1] = True
    elif pattern == 'every_1023rd':
        mask[::1023] = True
    elif pattern == 'half':
        mask[:] = np.random.default_rng(n).random(n) < 0.5
    else:
        assert pattern == 'none'
    return mask


@pytest.mark.parametrize('n_pairs, pattern', [(n, pattern) for n in (1023, 1024, 1025, 2049, 5000)
                                              for pattern in ('all', 'none', 'first', 'last', 'every_1023rd', 'half')])
def test_compaction_past_one_slot_per_thread(gpu_ctx, pool, n_pairs, pattern):
    """On the device entry slot p is pair p, so `first` and `last` are the compaction's first and last slot; the host entry
    compacts the same pairs through its own order (the `list` argument of the kernels)."""
    set1, set2, rows = pool
    positive = np.flatnonzero(rows[:, 0] > 0)
    index = positive[np.random.default_rng(n_pairs).integers(0, positive.size, n_pairs)]
    pair_a, pair_b, expected = index // 14, index % 14, rows[index].copy()
    passes = passing(pattern, n_pairs)
    min_score = (expected[:, 0] + np.where(passes, 0, 1)).astype(np.int32)
    expected[np.ix_(~passes, STATS_COLUMNS)] = 0
    assert (rows[index][:, 6] > 0).all()
    name = 'compact_%d_%s' % (n_pairs, pattern)
    got = run_host(gpu_ctx, name + '_host', set1, set2, pair_a, pair_b, min_score)
    assert gpu_ctx.sw_last_stats_pairs() == passes.sum()
    np.testing.assert_array_equal(got, expected)
    got, error = run_dev(gpu_ctx, name + '_dev', dev_arrays(set1, set2, pair_a, pair_b, min_score), len(set1), len(set2),
                         max(len(x) for x in set1 + set2), 0xFF)
    assert error is None and gpu_ctx.sw_last_stats_pairs() == passes.sum()
    np.testing.assert_array_equal(got, expected)


# ---- C4 .. C7: closed forms and the traceback ---------------------------------------------------------------------------------
def test_forced_ties_of_the_best_cell(gpu_ctx, ties):
    """The second cell of the best score lies in the same lane, the next lane, a far lane, the next strip or a later
    16-step block than the first; with min_score above the score only the score pass decides."""
    queries, subjects, rows, S = ties
    assert rows.shape == (28, 8) and (rows[:, 0] == S).all()
    np.testing.assert_array_equal(run_one_to_one(gpu_ctx, 'ties', queries, subjects), rows)
    assert gpu_ctx.sw_last_stats_pairs() == 28
    np.testing.assert_array_equal(run_one_to_one(gpu_ctx, 'ties_score_only', queries, subjects, S + 1), score_only_rows(rows))
    assert gpu_ctx.sw_last_stats_pairs() == 0


def test_one_gap_through_strip_boundaries(gpu_ctx, strip_gaps):
    """A gap of W or more residues along the query opens in one strip, fills the next and closes in a third: F and its
    statistics go through the workspace twice and the gap is still one opening."""
    queries, subjects, rows = strip_gaps
    assert rows.shape == (40, 8) and (rows[:, 7] == 1).all()
    np.testing.assert_array_equal(run_one_to_one(gpu_ctx, 'strip_gaps', queries, subjects), rows)


def test_late_starts_at_the_length_limit(gpu_ctx, late_starts):
    """Both halves of q_start << 16 | s_start are large, and n_ident << 16 | n_cols is not a homopolymer's."""
    queries, subjects, rows = late_starts
    np.testing.assert_array_equal(run_one_to_one(gpu_ctx, 'late_starts', queries, subjects), rows)


def test_two_letter_relatives_past_one_strip_against_the_traceback(gpu_ctx, two_letter):
    queries, subjects, rows = two_letter
    np.testing.assert_array_equal(run_one_to_one(gpu_ctx, 'two_letter', queries, subjects), rows)


# ---- C8: what the device entry refuses -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('bad', ['pair_a', 'pair_b', 'offsets'])
def test_the_device_entry_refuses_and_the_next_call_is_right(gpu_ctx, pool, bad):
    """The kernels skip such a pair (they read nothing that the offsets do not name) and the call fails."""
    set1, set2, rows = pool
    index = np.random.default_rng(12).integers(0, 196, 2000)
    good = dev_arrays(set1, set2, index // 14, index % 14, 1)
    arrays = [x.copy() for x in good]
    if bad == 'pair_a':
        arrays[4][1000] = len(set1)
    elif bad == 'pair_b':
        arrays[5][1000] = len(set2)
    else:
        # sequence 0 is empty and sequence 1 has one residue: offsets 0, 0, 1, ... become 0, 2, 1, ...; every offset still
        # lies inside the residues. Sequence 0 is then two residues long, not empty, so its pairs run a real alignment in
        # the refused call: in bounds, and that call's rows are not compared
        assert arrays[1][:3].tolist() == [0, 0, 1] and arrays[0].size > 2
        arrays[1][1] = 2
        assert (index // 14 == 1).any()
    max_len = max(len(x) for x in set1 + set2)
    _, error = run_dev(gpu_ctx, 'refused_' + bad, arrays, len(set1), len(set2), max_len, 0x5A)
    assert error is not None and REFUSED in str(error)
    got, error = run_dev(gpu_ctx, 'after_refused_' + bad, good, len(set1), len(set2), max_len, 0x5A)
    assert error is None
    np.testing.assert_array_equal(got, rows[index])
