"""The inputs of tests/cluster_band_sets.py do what tests/test_gpu_cluster_bands.py relies on -- shown with the CPU
oracle alone, no GPU. For a set whose only candidate pair is one (query, representative) pair the oracle's counters
describe that pair: aligned_pairs says whether it passed the diagonal test, dp_cells / len(query) is the width
band_right - band_left + 1 of its trimmed band, and the identity (or a second cluster) says how the alignment ended.
Every interesting pair of every generator runs through the oracle on its own, at each band width it is meant for.

These are conditions on the inputs, not measurements of the library: where one fails, the generator is to be changed."""
import collections

import numpy as np
import pytest

import cluster_band_sets as B
import oracle
from pangenomix_amd import cluster

Obs = collections.namedtuple('Obs', 'aligned width accepted identity stats')


def run_pair(bs, pair, band_width):
    """The pair alone, longer sequence first (the representative), through the oracle."""
    a, b = bs.seqs[pair.rep], bs.seqs[pair.query]
    if len(b) > len(a):
        a, b = b, a
    res, off = B.pack([a, b])
    p = cluster.params_from_cdhit_args(dict(bs.args, **{'-b': band_width}), bs.alphabet)
    cl, mem, iden, strand, nc, st = oracle.cluster_greedy(res, off, p)
    n_b = sum(ch.isalpha() for ch in b)
    width = st['dp_cells'] / n_b if st['aligned_pairs'] == 1 else None     # (both strands tried: no single band)
    return Obs(st['aligned_pairs'], width, nc == 1, float(iden[1]), st)


@pytest.fixture(scope='module')
def observed():
    out = {}
    for name, make in B.ALL_SETS.items():
        bs = make()
        for pair in bs.pairs:
            for w in pair.widths:
                out[name, pair.label, w] = run_pair(bs, pair, w)
    return out


def test_sets_are_small_and_reproducible():
    for name, make in B.ALL_SETS.items():
        bs, again = make(), make()
        assert bs.seqs == again.seqs and bs.pairs == again.pairs, name
        assert len(bs.seqs) <= 300 and max(len(s) for s in bs.seqs) <= 4000, name
        assert len({p.label for p in bs.pairs}) == len(bs.pairs), name
        assert all(set(p.widths) <= set(B.BAND_WIDTHS) for p in bs.pairs), name


def test_every_band_width_class_is_reached(observed):
    """Trimmed bands of 1, 2..20, 21..32, 33..63 and 64 diagonals, and the two widths on either side of the hand-off
    from the 16-lane aligner to the general one (32 and 33), each by at least one aligned pair. No band exceeds the
    band width it was run with."""
    widths = collections.Counter()
    for (name, label, b), o in observed.items():
        if o.width is not None:
            assert o.width == int(o.width) and 1 <= o.width <= b, (name, label, b, o.width)
            widths[int(o.width)] += 1
    for lo, hi in ((1, 1), (2, 20), (21, 32), (33, 63), (64, 64), (32, 32), (33, 33)):
        assert any(lo <= w <= hi for w in widths), 'no aligned pair with a band of %d..%d diagonals' % (lo, hi)
    # ... and the hand-off is taken by SHORT pairs for their band, not their length: both sequences far below the
    # aligner's smallest slot
    for want in (32, 33, 64):
        assert any(o.width == want for (name, label, b), o in observed.items() if name in ('indel', 'nt indel')), want


@pytest.mark.parametrize('name', ['indel', 'nt indel'])
def test_every_indel_size_is_aligned_and_accepted_and_aligned_and_rejected(name, observed):
    for s in B.INDEL_SIZES:
        tag = ('indel %d ' if name == 'indel' else 'nt indel %d ') % s
        obs = [o for (n, label, b), o in observed.items() if n == name and label.startswith(tag)]
        assert any(o.aligned and o.accepted and o.identity >= np.float32(0.8) for o in obs), 'size %d: none accepted' % s
        assert any(o.aligned and not o.accepted for o in obs), 'size %d: none aligned and rejected' % s
        assert any(o.accepted and o.identity < 0.9 for o in obs) and any(o.accepted and o.identity > 0.95 for o in obs), s


def test_indels_beyond_the_band_change_the_outcome(observed):
    """What makes the band width matter: the same pair is rejected with a band that holds one side of the indel and
    accepted with one that holds both; two indels of the same sign need the band to hold their sum."""
    for s in (21, 31, 32, 33, 40):
        narrow, wide = observed['indel', 'indel %d mid' % s, 20], observed['indel', 'indel %d mid' % s, 64]
        assert not narrow.accepted and wide.accepted and wide.width > s, s
    for s in (19, 20, 21, 31, 32, 33):                       # the band width just below / at / above the indel
        got = {b: observed['indel', 'indel %d mid' % s, b].accepted for b in (s, s + 1) if ('indel', 'indel %d mid' % s, b) in observed}
        assert got.get(s) is not True and got.get(s + 1) is not False and got, (s, got)
    assert not observed['indel', 'two indels 31 same sign', 20].accepted
    assert observed['indel', 'two indels 31 same sign', 63].accepted and observed['indel', 'two indels 31 same sign', 63].width == 63
    assert observed['indel', 'two indels 31 opposite', 64].accepted


def test_every_tie_is_observable(observed):
    """A tie pair and its mirror image (both sequences reversed) hold the same blocks in the opposite order. Were the
    rules 'first best window' and 'a tie keeps the earlier diagonal' without effect, the two would come out alike;
    they must differ in identity or in a counter, at a band width the pair is meant for."""
    bs = B.tie_pairs()
    seen = 0
    for p in bs.pairs:
        if p.label.endswith(', mirror'):
            continue
        differ = False
        for b in p.widths:
            o, m = observed['tie', p.label, b], observed['tie', p.label + ', mirror', b]
            assert o.aligned and m.aligned, (p.label, b)
            differ |= o.identity != m.identity or o.stats != m.stats
        assert differ, p.label                              # (at one of the band widths the pair is meant for)
        seen += 1
    assert seen >= 10
    # the constructed ties, by their known answers (cluster_band_sets.tie_in_window_pair / tie_of_windows_pair)
    o, m = observed['tie', 'in window, gap 5', 20], observed['tie', 'in window, gap 5, mirror', 20]
    assert (o.width, m.width) == (11, 16) and o.identity == np.float32(40) / np.float32(48) and m.identity == 1.0
    for n in (60, 120):
        first, last = observed['tie', 'windows, n %d, larger first' % n, 20], observed['tie', 'windows, n %d, larger last' % n, 20]
        assert first.identity == np.float32(n - 3) / np.float32(n) and last.identity == np.float32(n - 5) / np.float32(n)
        assert first.width == last.width == 1


def test_long_scans_reach_every_lane_class(observed):
    """The window scan of the long pairs gives every lane a stretch of several start positions and leaves the last
    lanes empty; the short ones have fewer windows than lanes, or none after the first. Every pair is found (aligned
    and accepted): its matching diagonal is where the generator put it."""
    bs = B.long_scan_pairs()
    pers, short_T = set(), set()
    for p in bs.pairs:
        o = observed['long scan', p.label, 20]
        assert o.aligned == 1 and o.accepted, p.label
        len2, len1 = len(bs.seqs[p.rep]), len(bs.seqs[p.query])
        band_b, band_m, T, per = B.scan_geometry(len1, len2, 20)
        if p.label.startswith('long'):
            assert 1500 <= len1 <= 4000 and per > 1 and 64 * per - T >= per, p.label     # at least one empty lane
            pers.add(per)
        else:
            short_T.add(T)
    assert len(pers) >= 4 and 0 in short_T and any(0 < T < 64 for T in short_T)
    labels = ' '.join(p.label for p in bs.pairs)
    for where in ('first lane', 'boundary', 'before boundary', 'last lane', 'last window', 'decoy'):
        assert where in labels


def test_no_input_reaches_the_refusal_of_a_band_wider_than_64():
    """The library refuses a pair whose trimmed band exceeds 64 diagonals (E_BAND, "alignment band wider than 64
    diagonals"). The oracle has no such rule, and neither side can produce such a band from a band width it accepts:
    diag_test starts from a window of min(band_width, len1 + len2 - 2) diagonals, a later best window has the same
    number, and the two trimming loops only ever move `from` up and `end` down. The trimmed band is therefore never
    wider than band_width <= 64 (asserted for every pair above), so no input provokes the refusal and the GPU suite
    has no case for it; the library's band_width > 64 refusal is what tests/test_gpu_cluster.py checks."""
    for bad in (0, 65):
        with pytest.raises(ValueError, match='-b'):
            cluster.params_from_cdhit_args({'-n': 5, '-c': 0.8, '-b': bad})
