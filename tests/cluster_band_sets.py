"""TEST INFRASTRUCTURE: seeded inputs for the band selection of greedy clustering (the diagonal test that picks a
window of `band_width` diagonals, its centre and its trimmed edges, and the banded aligners behind it). Pure
Python / numpy, no GPU, no oracle: tests/test_cluster_bands_host.py proves with the oracle's counters that these
inputs reach the band classes the GPU tests (tests/test_gpu_cluster_bands.py) rely on.

Every generator returns a BandSet: the sequences, the cd-hit style arguments to run them with, and the interesting
(representative, query) pairs as indices into the sequences, each with a label and the band widths it is meant for.

Vocabulary (oracle/cluster_ref.c, diag_test): a shared k-mer of query position i and representative position j lies
on diagonal len1 - 1 + (j - i); "offset" below is j - i. band_b = int(c * len1) - 1 is the first diagonal read, the
first window is band_b .. band_b + band_width - 1, and T = len1 + len2 + 1 - 2 int(c * len1) - band_width further
windows follow it.
"""
import collections

import numpy as np

AA = 'ACDEFGHIKLMNPQRSTVWY'
NT = 'ACGT'
BAND_WIDTHS = (1, 2, 19, 20, 21, 32, 33, 63, 64)          # every -b the GPU tests run
INDEL_SIZES = (1, 2, 5, 19, 20, 21, 31, 32, 33, 40, 63)

BandSet = collections.namedtuple('BandSet', 'name alphabet args seqs pairs')
Pair = collections.namedtuple('Pair', 'label rep query widths')


def rand_seq(rng, n, letters=AA):
    return ''.join(rng.choice(list(letters), size=n)) if n else ''


def revcomp(s):
    return s[::-1].translate(str.maketrans('ACGTN', 'TGCAN'))


def substitute(rng, s, positions, letters=AA):
    """Another letter at every given position (never the same one)."""
    s = list(s)
    for p in positions:
        others = [c for c in letters if c != s[p]]
        s[p] = others[int(rng.integers(0, len(others)))]
    return ''.join(s)


def scattered(rng, s, n_sub, letters=AA, keep=()):
    """n_sub single substitutions at random positions outside the `keep` ranges."""
    free = [p for p in range(len(s)) if not any(a <= p < b for a, b in keep)]
    return substitute(rng, s, rng.choice(free, size=min(n_sub, len(free)), replace=False), letters)


def blocks(rng, s, n_blocks, block_len, letters=AA):
    """n_blocks runs of block_len substitutions, evenly spaced: a run of k costs k identities but only k + 1 of the
    2-mers (k + 3 of the 4-mers), so such a member passes the diagonal test at identities where scattered
    substitutions fail it -- which is what gets a pair ALIGNED and then rejected."""
    step = len(s) // (n_blocks + 1)
    pos = [b * step + t for b in range(1, n_blocks + 1) for t in range(block_len)]
    return substitute(rng, s, [p for p in pos if p < len(s)], letters)


def apply_indels(rng, s, indels, letters=AA):
    """indels: (position in `s`, delta); delta > 0 inserts that many random residues before the position, delta < 0
    deletes that many from it on. Applied from the right, so every position refers to `s` itself."""
    for pos, delta in sorted(indels, reverse=True):
        s = s[:pos] + rand_seq(rng, delta, letters) + s[pos:] if delta > 0 else s[:pos] + s[pos - delta:]
    return s


def indel_family(rng, length, edits, letters=AA):
    """A base sequence of `length` residues and one member per entry of `edits`. An entry is (subs, indels):
    subs = ('scattered', n) or ('blocks', n_blocks, block_len) or None, applied to the base first; indels as in
    apply_indels. Returns [base, member, ...]."""
    base = rand_seq(rng, length, letters)
    out = [base]
    for subs, indels in edits:
        m = base
        if subs and subs[0] == 'scattered':
            m = scattered(rng, m, subs[1], letters)
        elif subs:
            m = blocks(rng, m, subs[1], subs[2], letters)
        out.append(apply_indels(rng, m, indels, letters))
    return out


def _indel_edits(L, s, sign):
    """The members of one family around an indel of s residues (sign: +1 insertion, -1 deletion in the member).
    Identities on both sides of 0.8, with the band holding both diagonals or only one of them."""
    d = sign * s
    few = ('scattered', max(2, L // 40))
    return [
        ('mid', (few, [(L // 2, d)])),                      # accepted iff the band holds both diagonals
        ('mid other sign', (few, [(L // 2 + 7, -d)])),
        ('near end', (few, [(L - L // 9, d)])),             # the far side holds a few hits only: trimming decides
        ('near start', (few, [(L // 10, d)])),
        ('two thirds', (('scattered', 3), [(L * 7 // 10, d)])),   # one side alone passes the diagonal test, not the threshold
        ('mid 0.78', (('blocks', 11, max(1, round(L * 0.22 / 11))), [(L // 2, d)])),   # aligned, then rejected
        ('mid 0.85', (('blocks', 11, max(1, round(L * 0.15 / 11))), [(L // 2, d)])),   # aligned, accepted
        ('mid 0.70', (('scattered', L * 3 // 10), [(L // 2, d)])),                      # fails the diagonal test
    ]


def indel_set(seed=101):
    """Protein families around one indel of every size of INDEL_SIZES, and around two indels of opposite sign (the
    hits return to the main diagonal) and of the same sign (they move further away)."""
    rng = np.random.default_rng(seed)
    seqs, pairs = [], []

    def add_family(tag, L, named_edits, widths):
        fam = indel_family(rng, L, [e for _, e in named_edits])
        b = len(seqs)
        seqs.extend(fam)
        for k, (name, _) in enumerate(named_edits):
            pairs.append(Pair('%s %s' % (tag, name), b, b + 1 + k, widths(name)))

    for k, s in enumerate(INDEL_SIZES):
        L = 330 if s < 33 else 420                          # (1 - c) * L + 1 >= s: the trimming keeps a band of s + 1
        add_family('indel %d' % s, L + 3 * k, _indel_edits(L + 3 * k, s, 1 if k % 2 else -1),
                   lambda name, s=s: (tuple(sorted({20, 64} | {b for b in BAND_WIDTHS if s <= b <= s + 2})) if name == 'mid'
                                      else (20, 64) if name == 'near end' else (64,) if name[:5] == 'mid 0' else (20,)))
    for s in (5, 19, 31):
        L = 400
        few = ('scattered', 8)
        add_family('two indels %d' % s, L + s, [
            ('opposite', (few, [(L // 3, s), (2 * L // 3, -s)])),
            ('opposite mirrored', (few, [(L // 3, -s), (2 * L // 3, s)])),
            ('same sign', (few, [(L // 3, -s), (2 * L // 3, -s)])),
            ('same sign ins', (few, [(L // 3, s), (2 * L // 3, s)])),
            ('same sign 0.78', (('blocks', 11, 8), [(L // 3, -s), (2 * L // 3, -s)])),
        ], lambda name, s=s: (20, 64) if s < 31 or name[:4] != 'same' else (20, 63, 64))
    return BandSet('indel', 'aa', {'-n': 5, '-c': 0.8}, seqs, pairs)


def nt_indel_set(seed=202):
    """The nucleotide counterpart: 4-mer diagonal test, members on either strand, a few N's next to the indel."""
    rng = np.random.default_rng(seed)
    seqs, pairs = [], []
    for k, s in enumerate(INDEL_SIZES):
        L = 340 + 3 * k if s < 33 else 430 + 3 * k
        d = s if k % 2 else -s
        few = ('scattered', L // 40)
        named = [
            ('mid', (few, [(L // 2, d)])),
            ('near end', (few, [(L - L // 9, d)])),
            ('near start', (few, [(L // 10, -d)])),
            ('mid 0.64', (('blocks', 11, max(1, round(L * 0.36 / 11))), [(L // 2, d)])),   # (a run of substituted
            ('mid 0.84', (('blocks', 11, max(1, round(L * 0.16 / 11))), [(L // 2, d)])),   # bases regains a quarter by chance)
        ]
        fam = indel_family(rng, L, [e for _, e in named], NT)
        for m in range(1, len(fam)):
            pos = named[m - 1][1][1][0][0]
            pos = min(pos, len(fam[m]) - 8)
            if m % 2:                                       # N's inside the indel neighbourhood
                fam[m] = fam[m][:pos - 3] + 'N' + fam[m][pos - 2:pos + 4] + 'NN' + fam[m][pos + 6:]
            if (m + k) % 3 == 0:                            # found on the reverse strand only
                fam[m] = revcomp(fam[m])
        b = len(seqs)
        seqs.extend(fam)
        for m, (name, _) in enumerate(named):
            widths = tuple(sorted({20, 64} | {w for w in BAND_WIDTHS if s <= w <= s + 2})) if name == 'mid' else (64,)
            pairs.append(Pair('nt indel %d %s' % (s, name), b, b + 1 + m, widths))
    return BandSet('nt indel', 'nt', {'-n': 5, '-c': 0.8}, seqs, pairs)


# ---- ties -------------------------------------------------------------------------------------------------
def clean_block(rng, letters, n):
    """n residues over `letters` in which no 2-mer occurs twice and no residue follows itself: matched against a
    copy of itself the block puts n - 1 hits of weight 2 on ONE diagonal and none anywhere else, so blocks over
    disjoint letters give a diagonal histogram that is known exactly."""
    letters = list(letters)
    while True:
        s, seen = [letters[int(rng.integers(0, len(letters)))]], set()
        while len(s) < n:
            cands = [c for c in letters if c != s[-1] and (s[-1], c) not in seen]
            if not cands:
                break
            c = cands[int(rng.integers(0, len(cands)))]
            seen.add((s[-1], c))
            s.append(c)
        if len(s) == n:
            return ''.join(s)


def tie_in_window_pair(rng, satellite_gap=5):
    """Two diagonals tie INSIDE a window. Query M1 M2 S, representative M1 x1 M2 x2 S with |M1| = |M2| = 20 (19 hits
    of weight 2 each: an exact tie), |S| = 8, |x1| = 10, |x2| = satellite_gap, all five parts over disjoint letters.
    At -c 0.8 -b 20 (len1 = 48, band_b = 37, first window 37..56): M1 lies on diagonal 47 inside the first window,
    M2 on 57 enters later and improves the window, with a weighted value EQUAL to the largest so far -- the centre
    stays on M1 ("a tie keeps the earlier diagonal"). Around M1 the trimming reaches emax = 10 diagonals: M2 stays,
    S (15 away) goes. With the centre on M2, S (satellite_gap away) would stay. The mirror image (both sequences
    reversed) meets S and M2 first, keeps the centre on M2, and keeps all three."""
    m1 = clean_block(rng, AA[0:6], 20)
    m2 = clean_block(rng, AA[6:12], 20)
    s = clean_block(rng, AA[12:16], 8)
    x1, x2 = clean_block(rng, AA[16:20], 10), clean_block(rng, AA[16:20], satellite_gap)
    return m1 + x1 + m2 + x2 + s, m1 + m2 + s


def tie_of_windows_pair(rng, n, larger_first):
    """Two WINDOWS tie. Query Q (n residues, clean over 16 letters); representative Q1 X Q2 where Q1 is Q with three
    single substitutions and Q2 is Q with one run of five: either costs six 2-mers, so the two diagonals (0 and
    n + |X| apart from it) carry the same hits and the same weighted hits, and every window that holds one of them
    scores the same. "First best window" then decides whether the query is aligned with Q1 (n - 3 identities) or
    with Q2 (n - 5). larger_first: Q1 first; otherwise Q2 first."""
    q = clean_block(rng, AA[:16], n)
    sub = AA[16:]
    q1 = substitute(rng, q, [n // 5, n // 2, n - n // 5], sub)
    q2 = substitute(rng, q, range(n // 2 - 2, n // 2 + 3), sub)
    x = rand_seq(rng, 10, sub)
    return (q1 + x + q2 if larger_first else q2 + x + q1), q


def tie_pairs(seed=303):
    """Pairs whose windows, or whose diagonals inside a window, tie exactly, each with its mirror image."""
    rng = np.random.default_rng(seed)
    seqs, pairs = [], []

    def add(label, rep, query, widths=(20,)):
        seqs.extend([rep, query])
        pairs.append(Pair(label, len(seqs) - 2, len(seqs) - 1, widths))

    for gap in (5, 9):                                      # 9: M1 .. S span 20 diagonals, the whole window
        rep, q = tie_in_window_pair(rng, gap)
        add('in window, gap %d' % gap, rep, q, (20,))
        add('in window, gap %d, mirror' % gap, rep[::-1], q[::-1], (20,))
    for n in (60, 120):                                     # 60: the first window holds the diagonal; 120: a later one
        for first in (True, False):
            rep, q = tie_of_windows_pair(rng, n, first)
            add('windows, n %d, %s' % (n, 'larger first' if first else 'larger last'), rep, q, (20,))
            add('windows, n %d, %s, mirror' % (n, 'larger first' if first else 'larger last'), rep[::-1], q[::-1], (20,))
    # low complexity: many diagonals carry hits, and homodimers weigh 1 where other 2-mers weigh 2
    r1 = rand_seq(rng, 30)
    low = [
        ('AC repeat', 'AC' * 60 + r1, 'AC' * 45 + r1[:12]),
        ('AC repeat shifted', r1 + 'CA' * 55, r1[20:] + 'AC' * 40),
        ('homopolymer interrupted', 'A' * 50 + 'C' + 'A' * 64, 'A' * 20 + 'C' + 'A' * 60),
        ('homopolymer and block', 'K' * 33 + r1 + 'K' * 25 + 'W' + 'K' * 50, 'K' * 22 + r1 + 'K' * 18 + 'W' + 'K' * 12),
    ]
    for label, rep, q in low:
        add('low complexity, %s' % label, rep, q, (20, 32))
        add('low complexity, %s, mirror' % label, rep[::-1], q[::-1], (20, 32))
    return BandSet('tie', 'aa', {'-n': 5, '-c': 0.8}, seqs, pairs)


# ---- long scans -------------------------------------------------------------------------------------------
def scan_geometry(len1, len2, band_width, c=0.8):
    """(band_b, band_m, T, per) of the window scan for a pair: T windows follow the first, 64 lanes take
    per = ceil(T / 64) consecutive start positions each; lane l owns t = 1 + l * per .. l * per + per."""
    nall = len1 + len2 - 1
    band_b = max(int(c * len1) - 1, 0)
    band_e = nall - band_b
    bw = min(band_width, len1 + len2 - 2)
    band_m = min(band_b + bw - 1, band_e)
    T = max(band_e - band_m - 1, 0) if band_m >= band_b else 0
    return band_b, band_m, T, (T + 63) // 64


def pair_on_offset(rng, len1, len2, offset, n_sub, letters=AA):
    """A representative of len2 residues and a query of len1 whose residue i equals the representative's residue
    i + offset wherever that exists (random elsewhere), with n_sub scattered substitutions inside the overlap."""
    rep = rand_seq(rng, len2, letters)
    q = list(rand_seq(rng, len1, letters))
    lo, hi = max(0, -offset), min(len1, len2 - offset)
    q[lo:hi] = rep[lo + offset:hi + offset]
    q = ''.join(q)
    return rep, substitute(rng, q, lo + rng.choice(hi - lo, size=n_sub, replace=False), letters)


def long_scan_pairs(seed=404, band_width=20):
    """Long pairs whose best window is first reached at a chosen start position t of the scan (the window's last
    diagonal, band_m + t, is the matching one), and short pairs with empty lanes or no later window at all."""
    rng = np.random.default_rng(seed)
    seqs, pairs = [], []

    def add(label, rep, query, widths=(band_width,)):
        seqs.extend([rep, query])
        pairs.append(Pair(label, len(seqs) - 2, len(seqs) - 1, widths))

    for len1, len2 in ((1500, 1700), (2300, 2300), (3100, 4000), (3800, 4000)):
        band_b, band_m, T, per = scan_geometry(len1, len2, band_width)
        assert per > 1 and 64 * per - T >= per, (T, per)     # stretches of several positions, and empty lanes at the end
        last_lane = (T - 1) // per
        targets = [('first lane', 2), ('first lane end', per), ('boundary', 1 + 7 * per), ('before boundary', 7 * per),
                   ('middle', 1 + 31 * per + per // 2), ('last lane', 1 + last_lane * per), ('last window', T)]
        for name, t in targets:
            offset = band_m + t - (len1 - 1)
            if offset + len1 > len2 and min(len1, len2 - offset) < int(0.8 * len1):
                continue                                    # (the representative is too short to hold the overlap)
            overlap = min(len1, len2 - offset) - max(0, -offset)
            rep, q = pair_on_offset(rng, len1, len2, offset, min(overlap // 50, max(0, overlap - int(0.8 * len1))))
            add('long %d/%d %s t=%d' % (len1, len2, name, t), rep, q)
        # a weaker copy of part of the query in an EARLIER lane's stretch, the real match later: the scan improves twice
        rep, q = pair_on_offset(rng, len1, len2, 0, len1 // 20)
        early = band_m + 3 * per + 1 - (len1 - 1)            # offset of the decoy: start position 1 + 3 per
        rep = list(rep)
        a = len1 // 3
        rep[a + early:a + early + 200] = q[a:a + 200] if a + early >= 0 else rep[a + early:a + early + 200]
        add('long %d/%d decoy then match' % (len1, len2), ''.join(rep), q)
    # T < 64: lanes with an empty stretch; T = 0: the window is the whole range of diagonals
    for L in (11, 12, 13, 14, 30, 60, 100, 150):
        s = rand_seq(rng, L + 2)
        add('short %d identical' % L, s, s[:L])
        add('short %d shifted' % L, s, substitute(rng, s[2:], [L // 2]))
    return BandSet('long scan', 'aa', {'-n': 5, '-c': 0.8}, seqs, pairs)


ALL_SETS = {'indel': indel_set, 'nt indel': nt_indel_set, 'tie': tie_pairs, 'long scan': long_scan_pairs}


def pack(seqs):
    lens = np.array([len(s) for s in seqs], dtype=np.uint64)
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    np.cumsum(lens, out=off[1:])
    return np.frombuffer(''.join(seqs).encode(), dtype=np.uint8), off
