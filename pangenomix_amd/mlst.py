"""Multi-locus sequence typing by exact allele matching (the reference's pangenome_analysis.run_mlst, :402-453, shells out to
tseemann's `mlst`, Perl + BLAST, under a hard-coded path; here the alleles of a scheme are searched in every genome with one
exact multi-pattern scan on the device: csrc/pattern.hip).

A scheme is a directory in the layout tseemann/mlst and PubMLST use: <scheme>.txt, a TSV whose header is `ST`, the loci, then
optional metadata columns (clonal_complex, species, ...), and one <locus>.tfa FASTA per locus with records `>locus_N` or
`>locus-N`.

The rules of a call (call_alleles states them in full) are this implementation's: exact matches only, on either strand, a
nested allele suppressed by the found allele that contains it, several alleles of a locus reported as `n,m`. They are not
pinned against the Perl tool, which is not available to the tests; novel (`~n`) and partial (`n?`) alleles are not called."""
from __future__ import print_function

import collections
import os

import numpy as np
import pandas as pd

MLST_PATH_COUNTS = collections.Counter()        # 'device' / 'host' per genome

MAX_SEED = 32
NONE = 0xFFFFFFFF
_UPPER = bytes.maketrans(b'abcdefghijklmnopqrstuvwxyz', b'ABCDEFGHIJKLMNOPQRSTUVWXYZ')
_COMPLEMENT_FROM = b'ACGTWSRYMKN'
_COMPLEMENT = bytes.maketrans(_COMPLEMENT_FROM, b'TGCAWSYRKMN')
HIT_COLUMNS = ['genome', 'locus', 'allele', 'contig', 'start', 'strand', 'copies']

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


def _call_genome(scheme, pats, path, names, seqs, first, count, hits):
    """One genome's row (ST, then the call per locus) from the patterns' first / count; appends to hits unless None."""
    found = [[] for _ in scheme.loci]             # per locus: (number, sequence, forward, reverse)
    for li, number, seq, fwd, rev in pats.rows:
        if count[fwd] or (rev >= 0 and count[rev]):
            found[li].append((number, seq, fwd, rev))
    starts = np.concatenate([[0], np.cumsum([len(s) + 1 for s in seqs])]) if seqs else np.zeros(1, dtype=np.int64)
    calls, numbers = [], []
    for li, locus in enumerate(scheme.loci):
        kept = [a for a in found[li]
                if not any(len(b[1]) > len(a[1]) and a[1] in b[1] for b in found[li])]
        kept.sort(key=lambda a: a[0])
        calls.append(','.join(str(a[0]) for a in kept) if kept else '-')
        numbers.append(kept[0][0] if len(kept) == 1 else None)
        if hits is not None:
            for number, seq, fwd, rev in kept:
                strands = [('+', fwd)] + ([('-', rev)] if rev >= 0 and rev != fwd else [])
                for strand, k in strands:
                    if count[k]:
                        c = int(np.searchsorted(starts, int(first[k]), side='right')) - 1
                        hits.append((path, locus, number, names[c], int(first[k]) - int(starts[c]) + 1, strand, int(count[k])))
    st = scheme.profiles.get(tuple(numbers), '-') if None not in numbers else '-'
    return [st] + calls


def call_alleles(scheme, genome_fna_paths, ctx=None, return_hits=False):
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
    * Novel and partial alleles (`~n`, `n?` in tseemann's tool) are not called: a locus without an exact match is `-`. The
      substring rule and the `n,m` rule are this implementation's and are not pinned against that tool.

    return_hits=True returns (frame, hits): hits has one row per called allele and strand it occurs on -- genome, locus,
    allele, contig and start (the contig that holds the first occurrence in the joined text and the 1-based position in it;
    on the minus strand the position where the reverse complement begins), strand, copies (occurrences on that strand in the
    whole genome). It is built from the scan's first / count and a searchsorted over the contig starts.

    ctx=None: the rules run on the host (host_scan), the statement of the rules, not a fast path. With a _native.Context: one
    pattern_load for the scheme and one pattern_query per genome, the next genome's FNA being parsed on a host thread meanwhile.
    A genome that holds a byte >= 0x80 is scanned by the host code. MLST_PATH_COUNTS counts the genomes of either path."""
    from concurrent.futures import ThreadPoolExecutor
    pats = _Patterns(scheme)
    paths = list(genome_fna_paths)
    rows, hits = [], [] if return_hits else None
    loaded = False
    with ThreadPoolExecutor(max_workers=1) as pool:
        ahead = pool.submit(read_genome, paths[0]) if paths else None
        for g, path in enumerate(paths):
            names, seqs = ahead.result()
            ahead = pool.submit(read_genome, paths[g + 1]) if g + 1 < len(paths) else None
            text = b'\x00'.join(seqs)
            if ctx is not None and pats.patterns and not text.translate(None, bytes(range(128))):
                if not loaded:
                    ctx.pattern_load(pats.blob, pats.offsets, seed=pats.seed)
                    loaded = True
                first, count = ctx.pattern_query(text)
                MLST_PATH_COUNTS['device'] += 1
            else:
                first, count = host_scan(text, pats.patterns, pats.seed)
                MLST_PATH_COUNTS['host'] += 1
            rows.append([path, scheme.name] + _call_genome(scheme, pats, path, names, seqs, first, count, hits))
    frame = pd.DataFrame(rows, columns=['genome', 'scheme', 'ST'] + list(scheme.loci))
    if return_hits:
        return frame, pd.DataFrame(hits, columns=HIT_COLUMNS)
    return frame


def format_mlst_line(path, scheme, st, loci, calls):
    """path <tab> scheme <tab> ST <tab> locus(call) ...: the line the external tool prints for a genome"""
    return '\t'.join([str(path), str(scheme), str(st)] + ['%s(%s)' % (locus, call) for locus, call in zip(loci, calls)])
