"""The prologue of a clustering call on the device: length histogram, stable descending-length order, offsets and
packed offsets of the sorted list (csrc/cluster.hip, "prep on the device"). Every case is compared with the CPU oracle
on all returned arrays and counters: a wrong order, a wrong offset or an unstable placement of equally long
sequences changes representatives, members or identities. Sets are small (a few thousand short sequences)."""
import numpy as np
import pytest

import oracle
from test_cluster_oracle import mutate, nt_params, pack, params, rand_nt, rand_seq, revcomp
from test_gpu_cluster import assert_same, assert_same_nt

pytestmark = pytest.mark.gpu

SORT_SHARE = 1024      # kSortShare: inputs per wave of the device sort
DEV_SORT_MAX = 65535   # kDevSortMaxLen: a longer sequence sends the whole call to the host's sort
HIST_LDS = 4096        # kHistLds: shorter lengths are counted in LDS first


def family_set(rng, lengths, count, per_family=6, max_sub=0.18):
    """`count` sequences whose lengths are drawn from `lengths`, in families of near copies of equal length,
    in shuffled order."""
    seqs = []
    while len(seqs) < count:
        L = int(rng.choice(lengths))
        base = rand_seq(rng, L)
        seqs.append(base)
        for _ in range(int(rng.integers(1, per_family))):
            seqs.append(mutate(rng, base, int(rng.integers(0, max(1, int(max_sub * L))))))
    seqs = seqs[:count]
    return [seqs[i] for i in rng.permutation(len(seqs))]


def check(gpu_ctx, seqs, p=None):
    p = p or params()
    res, off = pack(seqs)
    got = gpu_ctx.cluster_greedy(res, off, p)
    assert_same(got, oracle.cluster_greedy(res, off, p))
    return got


def test_ties_keep_input_order(gpu_ctx):
    """About ten distinct lengths, families inside the groups of equal length, shuffled: which of two equally long
    near copies becomes the representative depends on their input order alone."""
    rng = np.random.default_rng(101)
    seqs = family_set(rng, [41, 57, 58, 64, 90, 91, 120, 121, 150, 200], 3000)
    got = check(gpu_ctx, seqs)
    assert got[4] < len(seqs) // 2          # the families did form


@pytest.mark.parametrize('n_in', [63, 64, 65, SORT_SHARE - 1, SORT_SHARE, SORT_SHARE + 1,
                                  2 * SORT_SHARE - 1, 2 * SORT_SHARE, 2 * SORT_SHARE + 1])
def test_share_and_step_boundaries(n_in, gpu_ctx):
    """A wave of the sort takes 1024 inputs, 64 per step: one less, exactly and one more than a step, a share and
    two shares. Few distinct lengths, so that every step ranks ties and runs continue across shares."""
    rng = np.random.default_rng(1000 + n_in)
    seqs = family_set(rng, [30, 31, 44, 45, 60], n_in, per_family=4)
    assert len(seqs) == n_in
    check(gpu_ctx, seqs)


def test_letter_count_differs_from_byte_span(gpu_ctx):
    """The length of a record is its number of letters: '*', '-', digits, blanks are dropped, lower case counts.
    Records that tie only after the non-letters are dropped, an empty record, a record without any letter."""
    rng = np.random.default_rng(103)
    a, b, c = rand_seq(rng, 120), rand_seq(rng, 120), rand_seq(rng, 75)
    seqs = [
        a[:60] + '*' + a[60:] + '*',
        '',
        b,
        '--' + mutate(rng, a, 6).lower() + '--',
        '*-*--12345  ',
        c[:30] + '0123456789' + c[30:],
        mutate(rng, b, 5)[:50] + '-' * 70 + mutate(rng, b, 5)[50:],
        c.lower(),
        '-' + mutate(rng, c, 4),
        a[:119],
        '*' * 200,
        mutate(rng, a[:119], 3) + '*',
    ]
    seqs += ['-'.join(rand_seq(rng, 8) for _ in range(int(k))) for k in rng.integers(2, 12, 60)]
    got = check(gpu_ctx, seqs)
    assert got[0][1] == -1 and got[0][4] == -1 and got[0][10] == -1      # no letters: not clustered
    assert got[5]['n_clustered'] == len(seqs) - 3


def test_minimum_length(gpu_ctx):
    """Nothing longer than min_length: the call returns early with every record unclustered; then exactly one
    survivor (min_length is exclusive: 11 letters pass the default 10)."""
    rng = np.random.default_rng(104)
    short = [rand_seq(rng, int(k)) for k in rng.integers(0, 11, 200)]
    got = check(gpu_ctx, short)
    assert got[4] == 0 and (got[0] == -1).all()
    got = check(gpu_ctx, short[:100] + [rand_seq(rng, 11)] + short[100:])
    assert got[4] == 1 and got[0][100] == 0 and (np.delete(got[0], 100) == -1).all()
    got = check(gpu_ctx, [rand_seq(rng, int(k)) for k in rng.integers(20, 31, 300)], params(**{'-l': 30}))
    assert got[4] == 0
    check(gpu_ctx, [rand_seq(rng, int(k)) for k in rng.integers(20, 40, 300)], params(**{'-l': 30}))


def test_size_classes_of_the_word_lists_and_of_the_histogram(gpu_ctx):
    """The word-list kernels are chosen per run of the sorted list, from the histogram: lengths with exactly
    512/513, 1023/1024, 2048/2049 and 8192/8193 words (5-mers), each with a near copy that must find it, two of each
    length (ties); lengths on both sides of the histogram's LDS bins; ordinary short sequences around them."""
    rng = np.random.default_rng(105)
    seqs = []
    for words in (512, 513, 1023, 1024, 2048, 2049, 8192, 8193):
        s = rand_seq(rng, words + 4)
        seqs += [s, mutate(rng, s, max(3, words // 12)), rand_seq(rng, words + 4)]
    for L in (HIST_LDS - 1, HIST_LDS, HIST_LDS + 1):
        s = rand_seq(rng, L)
        seqs += [s, mutate(rng, s, 300)]
    seqs += family_set(rng, [100, 101, 250], 200)
    seqs = [seqs[i] for i in rng.permutation(len(seqs))]
    got = check(gpu_ctx, seqs)
    assert got[4] < len(seqs) - 10


@pytest.mark.parametrize('longest', [DEV_SORT_MAX, DEV_SORT_MAX + 1])
def test_both_sides_of_the_device_sort_bound(longest, gpu_ctx):
    """65,535 letters: the longest sequence the device sorts. One more and the whole call is ordered by the host. The
    same set otherwise, with ties and families, so both paths must give the same layout."""
    rng = np.random.default_rng(106)
    g = rand_seq(rng, longest)
    seqs = family_set(rng, [60, 61, 90], 300) + [g[:40000], g, mutate(rng, g, 2000)] + family_set(rng, [60, 75], 100)
    got = check(gpu_ctx, seqs)
    assert got[0][301] == got[0][302]


def test_both_strands_use_the_second_half_of_the_layout(gpu_ctx):
    """Nucleotides, both strands: the reverse complements are the virtual sequences n .. 2n-1, with offsets and packed
    offsets behind the first half's. Few distinct lengths, members that match on the reverse strand only."""
    rng = np.random.default_rng(107)
    seqs = []
    for L in (80, 81, 150, 150, 233, 400):
        for _ in range(12):
            a = rand_nt(rng, L)
            seqs += [a, revcomp(a), revcomp(a[:L - 1]) + 'N', a[:L - 3].lower() + '-' * 5 + a[L - 3:]]
    seqs = [seqs[i] for i in rng.permutation(len(seqs))]
    p = nt_params()
    res, off = pack(seqs)
    got = gpu_ctx.cluster_greedy(res, off, p)
    assert_same_nt(got, oracle.cluster_greedy(res, off, p))
    assert got[3].any()                                  # some joined on the reverse strand


def test_repeated_calls_on_one_context(gpu_ctx):
    """A larger set, then a smaller one with other lengths, each twice on the same context: histogram bins, sort
    counters or run tables left over from the call before would show."""
    rng = np.random.default_rng(108)
    big = family_set(rng, list(range(40, 400, 7)), 2500) + [rand_seq(rng, 5000)]
    small = family_set(rng, [33, 47, 48, 180], 300)
    p = params()
    want = {}
    for name, seqs in (('big', big), ('small', small)):
        res, off = pack(seqs)
        want[name] = (res, off, oracle.cluster_greedy(res, off, p))
    for name in ('big', 'small', 'small', 'big'):
        res, off, w = want[name]
        assert_same(gpu_ctx.cluster_greedy(res, off, p), w)
