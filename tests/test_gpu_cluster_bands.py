"""Greedy clustering on the GPU against the CPU oracle where the band selection and the banded aligners decide the
result: families with real insertions and deletions, pairs whose windows or diagonals tie, long pairs whose window
scan gives every lane a stretch of start positions, and every one of them at band widths from 1 to 64 -- the one
diagonal window, the widths around the hand-off from the 16-lane aligner to the general one (32 / 33), and the widest
band the library takes. Exact comparison: clusters, member numbers, float identities, strands, every counter.

tests/test_cluster_bands_host.py shows, with the oracle alone, which band classes these inputs reach. It also shows
why there is no case for the refusal of a band wider than 64 diagonals: no accepted band width can produce one."""
import numpy as np
import pytest

import cluster_band_sets as B
import oracle
from pangenomix_amd import cluster
from test_gpu_cluster import assert_same, assert_same_nt

pytestmark = pytest.mark.gpu

_sets, _wanted = {}, {}


def band_set(name):
    """(BandSet, residues, offsets) of a generator, its sequences in a fixed scrambled order."""
    if name not in _sets:
        bs = B.ALL_SETS[name]()
        order = np.random.default_rng(9).permutation(len(bs.seqs))
        _sets[name] = (bs,) + B.pack([bs.seqs[i] for i in order])
    return _sets[name]


def make_params(bs, batch_size=0, **args):
    p = cluster.params_from_cdhit_args(dict(bs.args, **args), bs.alphabet)
    p.batch_size = batch_size
    return p


def wanted(name, **args):
    """The oracle's result, computed once per (set, arguments): it does not depend on the window size."""
    key = (name,) + tuple(sorted(args.items()))
    if key not in _wanted:
        bs, res, off = band_set(name)
        _wanted[key] = oracle.cluster_greedy(res, off, make_params(bs, **args))
    return _wanted[key]


def check(gpu_ctx, name, **args):
    """Windows of the default size (families inside one window) and of 64 (older representatives: the 'short query,
    older representative' route), each with counters -- against the oracle -- and without -- the same four outputs."""
    bs, res, off = band_set(name)
    want = wanted(name, **args)
    same = assert_same_nt if bs.alphabet == 'nt' else assert_same
    for batch_size in (0, 64):
        p = make_params(bs, batch_size, **args)
        got = gpu_ctx.cluster_greedy(res, off, p)
        if bs.alphabet != 'nt':
            np.testing.assert_array_equal(got[3], want[3])
        same(got, want)
        lean = gpu_ctx.cluster_greedy(res, off, p, want_stats=False)
        assert lean[5] is None and lean[4] == got[4]
        for i in range(4):
            np.testing.assert_array_equal(lean[i], got[i])
    return want


@pytest.mark.parametrize('band_width', B.BAND_WIDTHS)
@pytest.mark.parametrize('name', sorted(B.ALL_SETS))
def test_matches_oracle_at_every_band_width(name, band_width, gpu_ctx):
    want = check(gpu_ctx, name, **{'-b': band_width})
    if band_width >= 20:
        assert want[5]['aligned_pairs'] >= len(band_set(name)[0].seqs) // 4
        assert 1 < want[4] < len(band_set(name)[0].seqs)          # members joined, and members were turned away


@pytest.mark.parametrize('args', [{'-c': 0.9}, {'-c': 0.7, '-n': 4}, {'-c': 0.9, '-b': 64}, {'-c': 0.7, '-n': 4, '-b': 64}],
                         ids=lambda a: ' '.join('%s %s' % kv for kv in sorted(a.items())))
@pytest.mark.parametrize('name', ['indel', 'tie'])
def test_matches_oracle_at_other_thresholds(name, args, gpu_ctx):
    """Another identity moves the first diagonal read (band_b = int(c * len) - 1) and the reach of the trimming
    (emax = int((1 - c) * mlen) + 1)."""
    check(gpu_ctx, name, **args)


def test_class_witness_pairs_one_at_a_time(gpu_ctx):
    """The pairs the host test names as witnesses of a band class or of a tie rule, each alone in its call, so that
    no other candidate stands between the query and the representative it is meant to meet: the ties with their known
    answers, and the indels of 31, 32, 33 and 63 residues at the band width that just holds them and at 64."""
    runs = []
    bs = B.tie_pairs()
    runs += [(bs, p, b) for p in bs.pairs for b in p.widths if not p.label.startswith('low')]
    bs = B.indel_set()
    runs += [(bs, p, b) for p in bs.pairs for b in p.widths
             if p.label in ('indel 31 mid', 'indel 32 mid', 'indel 33 mid', 'indel 63 mid', 'two indels 31 same sign') and b > 20]
    assert len(runs) >= 20
    widths = set()
    for bs, pair, b in runs:
        res, off = B.pack(sorted([bs.seqs[pair.rep], bs.seqs[pair.query]], key=len, reverse=True))
        p = make_params(bs, **{'-b': b})
        want = oracle.cluster_greedy(res, off, p)
        try:
            assert_same(gpu_ctx.cluster_greedy(res, off, p), want)
        except AssertionError as e:
            raise AssertionError('%s at -b %d: %s' % (pair.label, b, e))
        if want[5]['aligned_pairs'] == 1:
            widths.add(want[5]['dp_cells'] // int(off[2] - off[1]))
    assert {1, 11, 16, 32, 33, 63, 64} <= widths, sorted(widths)


def test_indel_families_on_two_virtual_ranks(monkeypatch):
    """The record-sharded path at a band width that sends pairs to both aligners."""
    from test_gpu_cluster_sharded import assert_replicated, fold, run_virtual_ranks
    bs, res, off = band_set('indel')
    p = make_params(bs, 64, **{'-b': 40})
    results = run_virtual_ranks(res, off, p, 2)
    assert_replicated(results)
    assert_same(fold(results), wanted('indel', **{'-b': 40}))
