"""Multi-locus sequence typing by allele matching (the reference's pangenome_analysis.run_mlst, :402-453, shells out to
tseemann's `mlst`, Perl + BLAST, under a hard-coded path; here the alleles of a scheme are searched in every genome with one
exact multi-pattern scan on the device: csrc/pattern.hip; and, on request, with one bounded-mismatch scan for
the loci that have no exact match: csrc/near.hip).

A scheme is a directory in the layout tseemann/mlst and PubMLST use: <scheme>.txt, a TSV whose header is `ST`, the loci, then
optional metadata columns (clonal_complex, species, ...), and one <locus>.tfa FASTA per locus with records `>locus_N` or
`>locus-N`.

The rules of a call (call_alleles states them in full) are this implementation's: exact matches only, on either strand, a
nested allele suppressed by the found allele that contains it, several alleles of a locus reported as `n,m`. They are not
pinned against the Perl tool, which is not available to the tests. With min_identity a locus without an exact match is called
`~n` for the allele nearest to a full-length ungapped window of the genome (Hamming distance within the identity threshold);
that search is exhaustive, where the tool's BLASTN additionally needs an exact 32-base word and ranks by bitscore. Partial
(`n?`) alleles are not called."""
from __future__ import print_function

import collections
import os

import numpy as np
import pandas as pd

MLST_PATH_COUNTS = collections.Counter()        # 'device' / 'host' per genome

MAX_SEED = 32
NONE = 0xFFFFFFFF
NEAR_NONE = 0xFFFFFFFFFFFFFFFF
NEAR_NO_SEPARATOR = 0x100
MAX_BLOCK = 32                                  # bytes of an indexed block of the near scan
MIN_DEVICE_BLOCK = 8                            # below it a block occurs by chance too often: the host handles the genome
_UPPER = bytes.maketrans(b'abcdefghijklmnopqrstuvwxyz', b'ABCDEFGHIJKLMNOPQRSTUVWXYZ')
_COMPLEMENT_FROM = b'ACGTWSRYMKN'
_COMPLEMENT = bytes.maketrans(_COMPLEMENT_FROM, b'TGCAWSYRKMN')
HIT_COLUMNS = ['genome', 'locus', 'allele', 'contig', 'start', 'strand', 'copies']
NEAR_HIT_COLUMNS = HIT_COLUMNS + ['mismatches']

Scheme = collections.namedtuple('Scheme', 'name loci alleles profiles')
Scheme.__doc__ = """name; loci in header order; alleles {locus: [(number, sequence as bytes), ...]} in file order; profiles
{(allele number per locus, ...): ST as a string}, the first line of a tuple given twice."""


def _fasta_records(path):
    """(line number of the header, header without '>', sequence bytes) of every record"""
    out = []
    with open(path, 'rb') as f:
        header, at, blocks = None, 0, []
        for n, line in enumerate(f, 1):
            line = line.strip()
            if line.startswith(b'>'):
                if header is not None:
                    out.append((at, header, b''.join(blocks)))
                header, at, blocks = line[1:], n, []
            elif header is not None:
                blocks.append(line)
        if header is not None:
            out.append((at, header, b''.join(blocks)))
    return out


def load_scheme(scheme_dir, scheme=None):
    """The scheme in `scheme_dir`: <scheme>.txt (the directory's only .txt when scheme is None) and the <locus>.tfa files.
    The loci are the header's columns behind `ST` up to the last one that has a .tfa file; the columns behind that one are
    metadata and are not read. ValueError, naming file and line: a column among the loci without a .tfa file, an allele
    record whose name is not <locus>_<number> or <locus>-<number>, a profile entry that is no number."""
    if scheme is None:
        tables = sorted(f for f in os.listdir(scheme_dir) if f.endswith('.txt'))
        if len(tables) != 1:
            raise ValueError('%s holds %d .txt files: name the scheme' % (scheme_dir, len(tables)))
        scheme = tables[0][:-4]
    table = os.path.join(scheme_dir, scheme + '.txt')
    with open(table, 'r') as f:
        lines = f.read().splitlines()
    if not lines or lines[0].split('\t')[0] != 'ST':
        raise ValueError('%s:1: the header must begin with ST' % table)
    columns = lines[0].split('\t')[1:]
    has = [os.path.isfile(os.path.join(scheme_dir, c + '.tfa')) for c in columns]
    if not any(has):
        raise ValueError('%s:1: no column has a .tfa file in %s' % (table, scheme_dir))
    n_loci = max(i for i, ok in enumerate(has) if ok) + 1
    loci = columns[:n_loci]
    for locus, ok in zip(loci, has):
        if not ok:
            raise ValueError('%s:1: locus %s has no file %s' % (table, locus, os.path.join(scheme_dir, locus + '.tfa')))
    alleles = {}
    for locus in loci:
        path = os.path.join(scheme_dir, locus + '.tfa')
        records = []
        for at, header, seq in _fasta_records(path):
            name = header.split()[0].decode('latin-1') if header.split() else ''
            number = name[len(locus) + 1:] if name[:len(locus)] == locus and name[len(locus):len(locus) + 1] in ('_', '-') else ''
            if not number.isdigit():
                raise ValueError('%s:%d: record %r is not %s_<number>' % (path, at, name, locus))
            records.append((int(number), seq))
        alleles[locus] = records
    profiles = {}
    for n, line in enumerate(lines[1:], 2):
        if not line.strip():
            continue
        cells = line.split('\t')
        try:
            key = tuple(int(c) for c in cells[1:1 + n_loci])
        except ValueError:
            key = ()
        if len(key) != n_loci:
            raise ValueError('%s:%d: a profile needs %d allele numbers' % (table, n, n_loci))
        profiles.setdefault(key, cells[0])
    return Scheme(scheme, loci, alleles, profiles)


def read_genome(path):
    """(contig names, contig sequences as bytes with a-z upper-cased) of an FNA file; records without sequence are left out"""
    names, seqs = [], []
    for _, header, seq in _fasta_records(path):
        if seq:
            names.append(header.split()[0].decode('latin-1') if header.split() else '')
            seqs.append(seq.translate(_UPPER))
    return names, seqs


class _Patterns(object):
    """The patterns of a scheme: every allele upper-cased, and its reverse complement where every character has a complement;
    equal byte strings share one pattern. rows: one per allele, (locus index, number, sequence, forward pattern, reverse
    pattern or -1)."""

    def __init__(self, scheme):
        index, rows = {}, []
        for li, locus in enumerate(scheme.loci):
            for number, seq in scheme.alleles[locus]:
                seq = seq.translate(_UPPER)
                if not seq:
                    raise ValueError('allele %s_%d is empty' % (locus, number))
                if b'\x00' in seq:
                    raise ValueError('allele %s_%d holds the byte 0x00' % (locus, number))
                fwd = index.setdefault(seq, len(index))
                rev = -1
                if not seq.translate(None, _COMPLEMENT_FROM):
                    rev = index.setdefault(seq.translate(_COMPLEMENT)[::-1], len(index))
                rows.append((li, number, seq, fwd, rev))
        self.rows = rows
        self.patterns = list(index)
        self.seed = min([MAX_SEED] + [len(p) for p in self.patterns])
        lengths = np.array([len(p) for p in self.patterns], dtype=np.uint64)
        self.offsets = np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(lengths, dtype=np.uint64)])
        self.blob = np.frombuffer(b''.join(self.patterns), dtype=np.uint8)


def host_scan(text, patterns, seed):
    """(first, count) uint32 [n] of the patterns in text, the way the device finds them: the distinct seeds (the first `seed`
    bytes) are indexed, every occurrence of a seed is located with bytes.find, and the patterns that begin with it are
    compared there."""
    first = np.full(len(patterns), NONE, dtype=np.uint32)
    count = np.zeros(len(patterns), dtype=np.uint32)
    by_seed = collections.OrderedDict()
    for k, p in enumerate(patterns):
        by_seed.setdefault(p[:seed], []).append(k)
    for head, members in by_seed.items():
        at = text.find(head)
        while at >= 0:
            for k in members:
                if text.startswith(patterns[k], at):
                    if count[k] == 0:
                        first[k] = at
                    count[k] += 1
            at = text.find(head, at + 1)
    return first, count


def max_mismatches(length, min_identity):
    """m(L) = (L * (10000 - round(min_identity * 100))) // 10000: the differing bytes a window of L bytes may hold"""
    if not 0 < min_identity <= 100:
        raise ValueError('min_identity must be in (0, 100]')
    return (int(length) * (10000 - int(round(min_identity * 100)))) // 10000


def host_near(text, patterns, max_mismatch, block, separator=0, active=None):
    """best uint64 [n] of the patterns in text -- mismatches << 32 | position of the best full-length window that holds no
    `separator` byte (NEAR_NO_SEPARATOR: none) and differs in at most max_mismatch[k] bytes, NEAR_NONE for none and for a
    pattern whose active[k] is 0 -- the way the device finds them: pattern k gives its first max_mismatch[k] + 1
    non-overlapping blocks of `block` bytes, every occurrence of a distinct block is located with bytes.find, and the windows
    it names are compared in numpy. ValueError when (max_mismatch[k] + 1) * block > len(pattern k)."""
    text = bytes(text)
    data = np.frombuffer(text, dtype=np.uint8)
    best = [NEAR_NONE] * len(patterns)
    by_block = collections.OrderedDict()
    arrays = {}
    for k, p in enumerate(patterns):
        if (int(max_mismatch[k]) + 1) * block > len(p):
            raise ValueError('pattern %d is shorter than its max_mismatch + 1 blocks' % k)
        if active is not None and not active[k]:
            continue
        arrays[k] = np.frombuffer(p, dtype=np.uint8)
        for j in range(int(max_mismatch[k]) + 1):
            by_block.setdefault(p[j * block:(j + 1) * block], []).append((k, j))
    for head, members in by_block.items():
        at = text.find(head)
        while at >= 0:
            for k, j in members:
                i, length = at - j * block, len(patterns[k])
                if i < 0 or i + length > len(text):
                    continue
                window = data[i:i + length]
                if separator != NEAR_NO_SEPARATOR and (window == separator).any():
                    continue
                d = int(np.count_nonzero(window != arrays[k]))
                if d <= int(max_mismatch[k]):
                    best[k] = min(best[k], (d << 32) | i)
            at = text.find(head, at + 1)
    return np.array(best, dtype=np.uint64)


def _call_genome(scheme, pats, path, names, seqs, first, count, hits, near=None):
    """One genome's row (ST, then the call per locus) from the patterns' first / count; appends to hits unless None. near: None,
    or active (uint8 per pattern) -> best (uint64 per pattern), asked once for the loci without an exact call."""
    found = [[] for _ in scheme.loci]             # per locus: (number, sequence, forward, reverse)
    for li, number, seq, fwd, rev in pats.rows:
        if count[fwd] or (rev >= 0 and count[rev]):
            found[li].append((number, seq, fwd, rev))
    starts = np.concatenate([[0], np.cumsum([len(s) + 1 for s in seqs])]) if seqs else np.zeros(1, dtype=np.int64)
    novel = {}                                    # locus index -> ((mismatches, -length, number), position, strand)
    missing = set(li for li in range(len(scheme.loci)) if not found[li]) if near is not None else set()
    if missing:
        active = np.zeros(len(pats.patterns), dtype=np.uint8)
        for li, number, seq, fwd, rev in pats.rows:
            if li in missing:
                active[fwd] = 1
                if rev >= 0:
                    active[rev] = 1
        best = near(active)
        for li, number, seq, fwd, rev in pats.rows:
            if li in missing:
                hit, strand = int(best[fwd]), '+'
                if rev >= 0 and int(best[rev]) < hit:
                    hit, strand = int(best[rev]), '-'
                key = (hit >> 32, -len(seq), number)
                if hit != NEAR_NONE and (li not in novel or key < novel[li][0]):
                    novel[li] = (key, hit & 0xFFFFFFFF, strand)
    extra = (0,) if near is not None else ()
    calls, numbers = [], []
    for li, locus in enumerate(scheme.loci):
        kept = [a for a in found[li]
                if not any(len(b[1]) > len(a[1]) and a[1] in b[1] for b in found[li])]
        kept.sort(key=lambda a: a[0])
        if li in novel:
            (mismatches, _, number), at, strand = novel[li]
            calls.append('~%d' % number)
            numbers.append(None)
            if hits is not None:
                c = int(np.searchsorted(starts, at, side='right')) - 1
                hits.append((path, locus, number, names[c], at - int(starts[c]) + 1, strand, 0, mismatches))
            continue
        calls.append(','.join(str(a[0]) for a in kept) if kept else '-')
        numbers.append(kept[0][0] if len(kept) == 1 else None)
        if hits is not None:
            for number, seq, fwd, rev in kept:
                strands = [('+', fwd)] + ([('-', rev)] if rev >= 0 and rev != fwd else [])
                for strand, k in strands:
                    if count[k]:
                        c = int(np.searchsorted(starts, int(first[k]), side='right')) - 1
                        hits.append((path, locus, number, names[c], int(first[k]) - int(starts[c]) + 1, strand, int(count[k]))
                                    + extra)
    st = scheme.profiles.get(tuple(numbers), '-') if None not in numbers else '-'
    return [st] + calls


def call_alleles(scheme, genome_fna_paths, ctx=None, return_hits=False, min_identity=None):
    """One row per genome: columns genome (the path), scheme, ST, then the call of every locus. The rules:

    * Contigs and alleles are upper-cased (a-z only) before anything else. A genome is its contigs joined by a 0x00 byte, so no
      match spans two contigs; an allele holding 0x00 raises ValueError.
    * The reverse strand is searched through the reverse complements of the alleles (ACGT and WSRYMKN); an allele with any
      other character has no reverse pattern. Equal byte strings (palindromes, an allele that is another's reverse complement,
      one sequence under two numbers) share one pattern. The seed of the scan is min(32, the shortest pattern).
    * An allele is found if it occurs, whole and exactly, on either strand. A found allele is suppressed iff its sequence is a
      proper substring of another found allele of the same locus. The call of a locus is `-` for none, `n` for one allele,
      `n,m,...` ascending by number for several (two copies that carry different alleles; two numbers with one sequence).
    * ST is the profile's ST when every locus has exactly one call and the tuple is in the table, else `-`.
    * min_identity=None: novel and partial alleles (`~n`, `n?` in tseemann's tool) are not called, a locus without an exact
      match is `-`. The substring rule and the `n,m` rule are this implementation's and are not pinned against that tool.

    With a number 0 < min_identity <= 100 (the tool's --minid; it defaults to 95 there) novel alleles are called as well:

    * Threshold: a window of L bytes may differ from an allele of L bytes in m(L) = (L * (10000 - round(min_identity * 100)))
      // 10000 bytes (max_mismatches; integers only). Bytes are compared as bytes: an N in the genome is a mismatch.
    * The exact scan and its rules run first and are unchanged; only a locus with no exact call is looked at further.
    * For such a locus the forward and reverse patterns of its alleles are searched in the genome for their best full-length
      window: no gaps, no 0x00 (so none across a contig joint), at most m(L) differing bytes; fewest mismatches, then the
      smallest position. The scheme's patterns are indexed once, by blocks of min(32, min over patterns of L // (m(L) + 1))
      bytes (host_near; pgx.h "Bounded-mismatch search").
    * An allele's hit is the better of its two patterns' windows, `+` before `-` when both are equal. The call of the locus is
      `~n` for the allele with the fewest mismatches, then the longer sequence, then the lowest number -- one allele only;
      `-` when no allele has a window. "Longer first" keeps the spirit of the substring rule: a near copy of an allele is not
      called through a shorter allele nested in it.
    * ST is `-` whenever a locus is `~n`.
    * These rules are this implementation's too and are not pinned against the tool: its BLASTN search additionally needs an
      exact 32-base word and ranks by bitscore, this search is the exhaustive one. Partial alleles (`n?`) are not called.

    return_hits=True returns (frame, hits): hits has one row per called allele and strand it occurs on -- genome, locus,
    allele, contig and start (the contig that holds the first occurrence in the joined text and the 1-based position in it;
    on the minus strand the position where the reverse complement begins), strand, copies (occurrences on that strand in the
    whole genome). It is built from the scan's first / count and a searchsorted over the contig starts. With min_identity the
    columns are NEAR_HIT_COLUMNS: `mismatches` is 0 on exact rows, and a novel call is one row -- contig, start and strand of
    its best window, its mismatches, and copies = 0: not counted for inexact hits.

    ctx=None: the rules run on the host (host_scan, host_near), the statement of the rules, not a fast path. With a
    _native.Context: one pattern_load for the scheme and one pattern_query per genome, the next genome's FNA being parsed on a
    host thread meanwhile; with min_identity one near_load for the scheme and one near_query per genome that has a locus
    without an exact call. A genome that holds a byte >= 0x80 is scanned by the host code, and with min_identity every genome
    is when the scheme gives a block under 8 bytes or an m(L) over 255. MLST_PATH_COUNTS counts the genomes of either path."""
    from concurrent.futures import ThreadPoolExecutor
    pats = _Patterns(scheme)
    paths = list(genome_fna_paths)
    rows, hits = [], [] if return_hits else None
    loaded = False
    near_m = near_block = None
    near_on_device = near_loaded = False
    if min_identity is not None and pats.patterns:
        near_m = [max_mismatches(len(p), min_identity) for p in pats.patterns]
        near_block = min([MAX_BLOCK] + [len(p) // (m + 1) for p, m in zip(pats.patterns, near_m)])
        near_on_device = near_block >= MIN_DEVICE_BLOCK and max(near_m) <= 255
    elif min_identity is not None:
        max_mismatches(0, min_identity)                                          # (the argument is checked all the same)
    with ThreadPoolExecutor(max_workers=1) as pool:
        ahead = pool.submit(read_genome, paths[0]) if paths else None
        for g, path in enumerate(paths):
            names, seqs = ahead.result()
            ahead = pool.submit(read_genome, paths[g + 1]) if g + 1 < len(paths) else None
            text = b'\x00'.join(seqs)
            on_device = ctx is not None and bool(pats.patterns) and not text.translate(None, bytes(range(128)))
            if on_device and near_m is not None and not near_on_device:
                on_device = False
            if on_device:
                if not loaded:
                    ctx.pattern_load(pats.blob, pats.offsets, seed=pats.seed)
                    loaded = True
                first, count = ctx.pattern_query(text)
                MLST_PATH_COUNTS['device'] += 1
            else:
                first, count = host_scan(text, pats.patterns, pats.seed)
                MLST_PATH_COUNTS['host'] += 1
            near = None
            if near_m is not None and on_device:
                def near(active):
                    nonlocal near_loaded
                    if not near_loaded:
                        ctx.near_load(pats.blob, pats.offsets, near_m, near_block)
                        near_loaded = True
                    return ctx.near_query(text, separator=0, active=active)
            elif near_m is not None:
                def near(active):
                    return host_near(text, pats.patterns, near_m, near_block, separator=0, active=active)
            rows.append([path, scheme.name] + _call_genome(scheme, pats, path, names, seqs, first, count, hits, near))
    frame = pd.DataFrame(rows, columns=['genome', 'scheme', 'ST'] + list(scheme.loci))
    if return_hits:
        return frame, pd.DataFrame(hits, columns=HIT_COLUMNS if min_identity is None else NEAR_HIT_COLUMNS)
    return frame


def format_mlst_line(path, scheme, st, loci, calls):
    """path <tab> scheme <tab> ST <tab> locus(call) ...: the line the external tool prints for a genome"""
    return '\t'.join([str(path), str(scheme), str(st)] + ['%s(%s)' % (locus, call) for locus, call in zip(loci, calls)])
