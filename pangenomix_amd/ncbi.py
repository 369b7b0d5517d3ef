"""Bidirectional protein search between two FASTA files (the reference's ncbi.bidirectional_blast, ncbi.py:255-336, shells
out to makeblastdb and blastp twice and cannot run: `__run_commands__` and `verbose` are undefined names, ncbi.py:316). Here
the two outfmt-6 reports come from one exhaustive Smith-Waterman per candidate pair on the device: csrc/sw.hip, DESIGN.md 6t.

The rules are this implementation's own, exact, and stated once in DESIGN.md 6t; host_sw is their model and the kernel
follows them. In short: BLOSUM62 over the 21 letter classes of csrc/cluster_tables.h, a gap of k residues costs 11 + k, one
best local alignment per pair whose statistics are carried through the recurrence (no traceback), a pair is a candidate if
the two sequences share one exact word of `word_size` residues over the classes, and a hit's E-value and bit score use the
gapped BLOSUM62 11/1 constants with NO length adjustment. Where this differs from BLAST, on purpose: one alignment per pair;
an exhaustive Smith-Waterman behind an exact-word seed instead of two-hit neighbourhood words with X-drop; no
composition-based statistics; no masking; the number formats are not pinned against BLAST either."""
from __future__ import print_function

import collections
import math
import os
import re
import time

import numpy as np
import pandas as pd

from .cluster import read_fasta_for_clustering

NCBI_PATH_COUNTS = collections.Counter()        # 'device' / 'host': aligned pairs by path

GAP_OPEN, GAP_EXTEND = 11, 1                    # a gap of k residues costs GAP_OPEN + k * GAP_EXTEND
LAMBDA, K = 0.267, 0.041                        # gapped BLOSUM62 11/1
DEFAULT_EVALUE = 1e-10                          # the reference's
DEFAULT_MAX_TARGET_SEQS = 500
DEFAULT_WORD_SIZE = 5
OUTFMT6_COLUMNS = ['qseqid', 'sseqid', 'pident', 'length', 'mismatch', 'gapopen', 'qstart', 'qend', 'sstart', 'send',
                   'evalue', 'bitscore']
SW_COLUMNS = ['score', 'q_start', 'q_end', 's_start', 's_end', 'n_ident', 'n_cols', 'n_gapopen']
_NEG = -(1 << 29)
_KNOWN_PARAMS = {'evalue', 'max_target_seqs', 'word_size', 'num_threads', 'matrix', 'gapopen', 'gapextend'}
_IDENT, _COL, _GAP = 1 << 40, 1 << 20, 1        # the three counts of a path in one int64 (each below 2^20)

_tables = None


def tables():
    """(class of letter 0..26, substitution score of two letters [27, 27]) from csrc/cluster_tables.h: letters A-Z are 0..25,
    26 is every other byte; the classes and BLOSUM62 are the clustering's (tests/test_cluster_tables.py ties them to the
    oracle's copy)."""
    global _tables
    if _tables is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'csrc', 'cluster_tables.h')
        text = open(path).read()
        aa = re.search(r'kAa2Idx\[26\]\s*=\s*\{([^}]*)\}', text, re.S).group(1)
        flat = re.search(r'#define PGXC_BLOSUM62_FLAT \{(.*?)\}', text, re.S).group(1)
        cls = np.array([int(x) for x in aa.replace('\\', ' ').split(',')] + [20], dtype=np.int64)
        blosum = np.array([int(x) for x in flat.replace('\\', ' ').split(',')], dtype=np.int32).reshape(21, 21)
        _tables = (cls, np.ascontiguousarray(blosum[cls][:, cls]))
    return _tables


def letters_of(seq):
    """Letter indices of a sequence (bytes, str or a uint8 array): A-Z and a-z are 0..25, every other byte is 26."""
    if isinstance(seq, str):
        seq = seq.encode('latin-1')
    if isinstance(seq, (bytes, bytearray, memoryview)):
        seq = np.frombuffer(bytes(seq), dtype=np.uint8)
    u = (np.asarray(seq, dtype=np.uint8).astype(np.int64) | 32) - 97
    return np.where((u >= 0) & (u < 26), u, 26)


def host_sw(q, s, stats=True):
    """The model of DESIGN.md 6t for one pair: int32 [8] = score, q_start, q_end, s_start, s_end, n_ident, n_cols, n_gapopen
    of the best local alignment of q and s (0-based inclusive positions); without `stats`, or with score 0, the five
    statistics are 0. Evaluated along anti-diagonals with numpy: every cell is a function of its three predecessors, so the
    order is free."""
    cls, sub = tables()
    ql, sl = letters_of(q), letters_of(s)
    m, n = ql.size, sl.size
    out = np.zeros(8, dtype=np.int32)
    if m == 0 or n == 0:
        return out
    # index i + 1 of an array is query position i on that anti-diagonal; everything outside the diagonal is the border
    H1, H2 = np.zeros(m + 1, dtype=np.int64), np.zeros(m + 1, dtype=np.int64)
    E1, F1 = np.full(m + 1, _NEG, dtype=np.int64), np.full(m + 1, _NEG, dtype=np.int64)
    zero = np.zeros(m + 1, dtype=np.int64)
    HP1 = HC1 = EP1 = EC1 = FP1 = FC1 = HP2 = HC2 = zero
    best, best_i, best_j, best_p, best_c = 0, 0, 0, 0, 0
    for d in range(m + n - 1):
        lo, hi = max(0, d - (n - 1)), min(m - 1, d)
        I = np.arange(lo, hi + 1)
        J = d - I
        k, up = slice(lo + 1, hi + 2), slice(lo, hi + 1)
        e_ext, e_open = E1[k] - GAP_EXTEND, H1[k] - GAP_OPEN - GAP_EXTEND
        f_ext, f_open = F1[up] - GAP_EXTEND, H1[up] - GAP_OPEN - GAP_EXTEND
        E, F = np.maximum(e_ext, e_open), np.maximum(f_ext, f_open)
        diag = H2[up]
        D = diag + sub[ql[I], sl[J]]
        H = np.maximum(np.maximum(D, E), np.maximum(F, 0))
        if stats:
            from_ext = e_ext >= e_open                                   # extension before opening
            EP, EC = np.where(from_ext, EP1[k], HP1[k]), np.where(from_ext, EC1[k] + _COL, HC1[k] + _COL + _GAP)
            from_ext = f_ext >= f_open
            FP, FC = np.where(from_ext, FP1[up], HP1[up]), np.where(from_ext, FC1[up] + _COL, HC1[up] + _COL + _GAP)
            start = diag == 0                                            # a diagonal step from H = 0 starts a path here
            HP = np.where(start, (I << 32) | J, HP2[up])
            HC = np.where(start, 0, HC2[up]) + _COL + (ql[I] == sl[J]) * _IDENT
            take = E > D                                                 # the diagonal before E, E before F
            HP, HC = np.where(take, EP, HP), np.where(take, EC, HC)
            take = F > np.maximum(D, E)
            HP, HC = np.where(take, FP, HP), np.where(take, FC, HC)
        top = int(H.max())
        if top > 0 and top >= best:
            c = int(np.argmax(H))                                        # the smallest i of this diagonal
            i, j = int(I[c]), int(J[c])
            if top > best or (i, j) < (best_i, best_j):
                best, best_i, best_j = top, i, j
                if stats:
                    best_p, best_c = int(HP[c]), int(HC[c])
        H2, HP2, HC2 = H1, HP1, HC1
        H1 = np.zeros(m + 1, dtype=np.int64); H1[k] = H
        E1 = np.full(m + 1, _NEG, dtype=np.int64); E1[k] = E
        F1 = np.full(m + 1, _NEG, dtype=np.int64); F1[k] = F
        if stats:
            HP1, HC1, EP1, EC1, FP1, FC1 = (zero.copy() for _ in range(6))
            HP1[k], HC1[k], EP1[k], EC1[k], FP1[k], FC1[k] = HP, HC, EP, EC, FP, FC
    out[0], out[2], out[4] = best, best_i, best_j
    if stats and best > 0:
        out[1], out[3] = best_p >> 32, best_p & 0xFFFFFFFF
        out[5], out[6], out[7] = best_c >> 40, (best_c >> 20) & 0xFFFFF, best_c & 0xFFFFF
    return out


def candidate_pairs(res1, off1, res2, off2, word_size=DEFAULT_WORD_SIZE):
    """(pair_a, pair_b) uint32, sorted by (a, b): every pair of a sequence a of set 1 and a sequence b of set 2 that share at
    least one exact word of word_size (3..6) residues, compared over the 21 letter classes. A host join: 5-bit word codes,
    sort, join, unique."""
    word_size = int(word_size)
    if not 3 <= word_size <= 6:
        raise ValueError('word_size %d out of range (3..6)' % word_size)
    cls, _ = tables()

    def words(res, off):
        off = np.asarray(off, dtype=np.int64)
        n = off.size - 1
        c = cls[letters_of(res)]
        total = c.size
        if total < word_size:
            return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
        code = np.zeros(total - word_size + 1, dtype=np.int64)
        for t in range(word_size):
            code |= c[t:total - word_size + 1 + t] << (5 * t)
        seq = np.repeat(np.arange(n, dtype=np.int64), np.diff(off))
        at = np.arange(total - word_size + 1, dtype=np.int64)
        inside = at + word_size <= off[1:][seq[:at.size]]                # the word ends in the sequence it begins in
        key = np.unique((code[inside] << 32) | seq[:at.size][inside])
        return key >> 32, key & 0xFFFFFFFF

    code1, seq1 = words(res1, off1)
    code2, seq2 = words(res2, off2)
    first, last = np.searchsorted(code2, code1, 'left'), np.searchsorted(code2, code1, 'right')
    count = last - first
    a = np.repeat(seq1, count)
    within = np.arange(int(count.sum()), dtype=np.int64) - np.repeat(np.cumsum(count) - count, count)
    b = seq2[np.repeat(first, count) + within]
    n2 = np.asarray(off2).size - 1
    key = np.unique(a * max(n2, 1) + b)
    return (key // max(n2, 1)).astype(np.uint32), (key % max(n2, 1)).astype(np.uint32)


def evalue_of(score, query_length, other_total):
    """E = K * len(query) * (total residues of the other set) * exp(-lambda * S): no length adjustment."""
    return K * np.asarray(query_length, dtype=np.float64) * float(other_total) * np.exp(-LAMBDA * np.asarray(score, dtype=np.float64))


def bits_of(score):
    return (LAMBDA * np.asarray(score, dtype=np.float64) - math.log(K)) / math.log(2.0)


def min_scores(len_a, len_b, total1, total2, evalue):
    """A score below which a pair is reported in neither direction, one short of the real-valued threshold so that rounding
    cannot lose a hit: whether a line is written is decided on evalue_of alone."""
    with np.errstate(divide='ignore'):
        forward = np.log(K * len_a.astype(np.float64) * max(total2, 1) / evalue) / LAMBDA
        reverse = np.log(K * len_b.astype(np.float64) * max(total1, 1) / evalue) / LAMBDA
    least = np.nan_to_num(np.minimum(forward, reverse), neginf=0.0, posinf=2.0 ** 30)
    return np.clip(np.ceil(least) - 1, 1, 2 ** 30).astype(np.int32)


def align_pairs(res1, off1, res2, off2, pair_a, pair_b, min_score, ctx=None):
    """int32 [n_pairs, 8] (SW_COLUMNS) of every pair, the statistics only where score >= min_score: on host_sw without a
    Context, else through Context.sw_pairs, with pairs that hold a sequence longer than pgx_sw_max_length() left to host_sw.
    NCBI_PATH_COUNTS counts the pairs of either path."""
    off1, off2 = np.asarray(off1, dtype=np.uint64), np.asarray(off2, dtype=np.uint64)
    pair_a, pair_b = np.asarray(pair_a, dtype=np.uint32), np.asarray(pair_b, dtype=np.uint32)
    min_score = np.ascontiguousarray(np.broadcast_to(np.asarray(min_score, dtype=np.int32), pair_a.shape))
    out = np.zeros((pair_a.size, 8), dtype=np.int32)
    on_host = np.ones(pair_a.size, dtype=bool)
    if ctx is not None and pair_a.size:
        from . import _native
        limit = int(_native.lib().pgx_sw_max_length())
        len1, len2 = np.diff(off1.astype(np.int64)), np.diff(off2.astype(np.int64))
        on_host = (len1[pair_a] > limit) | (len2[pair_b] > limit)
        dev = np.flatnonzero(~on_host)
        if dev.size:
            out[dev] = ctx.sw_pairs(res1, off1, res2, off2, pair_a[dev], pair_b[dev], min_score[dev])
            NCBI_PATH_COUNTS['device'] += int(dev.size)
    for p in np.flatnonzero(on_host).tolist():
        q = res1[int(off1[pair_a[p]]):int(off1[pair_a[p] + 1])]
        s = res2[int(off2[pair_b[p]]):int(off2[pair_b[p] + 1])]
        r = host_sw(q, s, stats=False)
        if r[0] > 0 and r[0] >= min_score[p]:
            r = host_sw(q, s, stats=True)
        out[p] = r
        NCBI_PATH_COUNTS['host'] += 1
    return out


def _report_lines(ids_q, ids_s, pair_q, pair_s, rows, swap, evalue_arr, max_target_seqs):
    """outfmt-6 lines of one direction. rows: SW_COLUMNS of the reported pairs with the set-1 sequence as q; swap: the
    report's query is the set-2 sequence."""
    order = np.lexsort((pair_s, -rows[:, 0].astype(np.int64), evalue_arr, pair_q))   # query, E, score descending, subject
    rank = np.arange(order.size) - np.searchsorted(pair_q[order], pair_q[order], 'left')
    lines = []
    for p in order[rank < max_target_seqs].tolist():
        score, qs, qe, ss, se, ident, cols, gaps = (int(x) for x in rows[p])
        mismatch = (qe - qs + 1) + (se - ss + 1) - cols - ident
        if swap:
            qs, qe, ss, se = ss, se, qs, qe
        lines.append('%s\t%s\t%.3f\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%.3g\t%.1f\n' % (
            ids_q[pair_q[p]], ids_s[pair_s[p]], 100.0 * ident / cols, cols, mismatch, gaps, qs + 1, qe + 1, ss + 1, se + 1,
            evalue_arr[p], bits_of(score)))
    return lines


def search_reports(ids1, res1, off1, ids2, res2, off2, evalue=DEFAULT_EVALUE, max_target_seqs=DEFAULT_MAX_TARGET_SEQS,
                   word_size=DEFAULT_WORD_SIZE, ctx=None, timings=None):
    """(forward lines, reverse lines) of two sets of proteins given as arrays (read_fasta_for_clustering's). Every candidate
    pair is aligned once, with the set-1 sequence as query; the reverse report lists the same alignment with query and
    subject exchanged. timings: a dict that receives the seconds of the join and of the alignment."""
    off1, off2 = np.asarray(off1, dtype=np.uint64), np.asarray(off2, dtype=np.uint64)
    t0 = time.perf_counter()
    pair_a, pair_b = candidate_pairs(res1, off1, res2, off2, word_size)
    t1 = time.perf_counter()
    len1, len2 = np.diff(off1.astype(np.int64)), np.diff(off2.astype(np.int64))
    total1, total2 = int(len1.sum()), int(len2.sum())
    rows = align_pairs(res1, off1, res2, off2, pair_a, pair_b,
                       min_scores(len1[pair_a], len2[pair_b], total1, total2, evalue), ctx=ctx)
    t2 = time.perf_counter()
    if timings is not None:
        timings.update(join_s=t1 - t0, align_s=t2 - t1, candidate_pairs=int(pair_a.size),
                       cells=int((len1[pair_a] * len2[pair_b]).sum()))
    forward_e = evalue_of(rows[:, 0], len1[pair_a], total2)
    reverse_e = evalue_of(rows[:, 0], len2[pair_b], total1)
    keep = np.flatnonzero((rows[:, 0] > 0) & (forward_e <= evalue))
    forward = _report_lines(ids1, ids2, pair_a[keep], pair_b[keep], rows[keep], False, forward_e[keep], max_target_seqs)
    keep = np.flatnonzero((rows[:, 0] > 0) & (reverse_e <= evalue))
    reverse = _report_lines(ids2, ids1, pair_b[keep], pair_a[keep], rows[keep], True, reverse_e[keep], max_target_seqs)
    return forward, reverse


def _search_params(blast_params):
    params = dict(blast_params or {})
    unknown = set(params) - _KNOWN_PARAMS
    if unknown:
        raise ValueError('unsupported blastp option(s): %s' % ', '.join(sorted(unknown)))
    if str(params.get('matrix', 'BLOSUM62')).upper() != 'BLOSUM62':
        raise ValueError('matrix %s: only BLOSUM62 is built' % params['matrix'])
    if int(params.get('gapopen', GAP_OPEN)) != GAP_OPEN or int(params.get('gapextend', GAP_EXTEND)) != GAP_EXTEND:
        raise ValueError('gap costs other than gapopen 11 / gapextend 1 are not built')
    if int(params.get('num_threads', 1)) != 1:
        print('Note: num_threads %s ignored: the alignments run on the device' % params['num_threads'])
    evalue = float(params.get('evalue', DEFAULT_EVALUE))
    if not evalue > 0:
        raise ValueError('evalue must be positive')
    max_target_seqs = int(params.get('max_target_seqs', DEFAULT_MAX_TARGET_SEQS))
    if max_target_seqs < 1:
        raise ValueError('max_target_seqs must be at least 1')
    return evalue, max_target_seqs, int(params.get('word_size', DEFAULT_WORD_SIZE))


def bidirectional_blast(seq1_fasta, seq2_fasta, report_dir, blast_params={'evalue': 0.0000000001, 'num_threads': 1},
                        seq1_blast_db=None, seq2_blast_db=None, ctx=None, timings=None):
    """Takes two protein FASTA files <strain>.faa and writes the two outfmt-6 reports of searching each against the other
    (reference ncbi.py:255-336): <report_dir>/<name1>_to_<name2>.tsv and <report_dir>/<name2>_to_<name1>.tsv. Returns
    (forward_report, reverse_report). The directories the reference creates are created and the two argument lists it prints
    are printed, but no BLAST database files are written and no program is started: the rules are the module's (DESIGN.md
    6s). blast_params: evalue, max_target_seqs and word_size (3..6) are honoured; num_threads is ignored with a note; matrix,
    gapopen and gapextend are accepted at BLOSUM62 / 11 / 1 only; any other key is a ValueError. A .fna input (the reference's
    blastn branch) is a ValueError: only proteins are built. ctx: a Context runs the alignments on the device, None on the
    host model; the reports are byte-identical."""
    if seq1_fasta[-4:] != '.faa' or seq2_fasta[-4:] != '.faa':
        raise ValueError('only protein searches (.faa against .faa) are built; the blastn branch for .fna files is not')
    evalue, max_target_seqs, word_size = _search_params(blast_params)
    if not 3 <= word_size <= 6:
        raise ValueError('word_size %d out of range (3..6)' % word_size)
    add_slash = lambda x: x if x[-1] == '/' else x + '/'
    get_file_dir = lambda x: '/'.join(x.split('/')[:-1]) + '/' if '/' in x else ''
    get_filename = lambda x: x.split('/')[-1]
    name1 = '.'.join(get_filename(seq1_fasta).split('.')[:-1])
    name2 = '.'.join(get_filename(seq2_fasta).split('.')[:-1])
    report_dir = add_slash(report_dir)
    forward_report = report_dir + name1 + '_to_' + name2 + '.tsv'
    reverse_report = report_dir + name2 + '_to_' + name1 + '.tsv'
    db1_dir = add_slash(seq1_blast_db) if seq1_blast_db else get_file_dir(seq1_fasta)
    db2_dir = add_slash(seq2_blast_db) if seq2_blast_db else get_file_dir(seq2_fasta)
    for directory in [report_dir, db1_dir, db2_dir]:
        if directory and not os.path.isdir(directory):
            os.mkdir(directory)
    extra_blast_args = []
    for param, value in (blast_params or {}).items():
        extra_blast_args += ['-' + str(param), str(value)]
    forward_args = ['blastp', '-db', db2_dir + get_filename(seq2_fasta), '-query', seq1_fasta, '-out', forward_report,
                    '-outfmt', '6'] + extra_blast_args
    reverse_args = ['blastp', '-db', db1_dir + get_filename(seq1_fasta), '-query', seq2_fasta, '-out', reverse_report,
                    '-outfmt', '6'] + extra_blast_args
    t0 = time.perf_counter()
    ids1, res1, off1, _ = read_fasta_for_clustering(seq1_fasta)
    ids2, res2, off2, _ = read_fasta_for_clustering(seq2_fasta)
    t1 = time.perf_counter()
    forward, reverse = search_reports(ids1, res1, off1, ids2, res2, off2, evalue, max_target_seqs, word_size, ctx=ctx,
                                      timings=timings)
    t2 = time.perf_counter()
    print(forward_args)
    with open(forward_report, 'w') as f:
        f.writelines(forward)
    print(reverse_args)
    with open(reverse_report, 'w') as f:
        f.writelines(reverse)
    if timings is not None:
        timings.update(read_s=t1 - t0, write_s=time.perf_counter() - t2)
    return forward_report, reverse_report


def read_report(path):
    """An outfmt-6 report as a DataFrame (OUTFMT6_COLUMNS; the ids as strings), lines in file order."""
    return pd.read_csv(path, sep='\t', header=None, names=OUTFMT6_COLUMNS, dtype={'qseqid': str, 'sseqid': str})


def reciprocal_best_hits(forward_report, reverse_report):
    """The pairs that are each other's first line: a DataFrame with one row per pair (seq1, seq2, then pident, length, evalue
    and bitscore of the forward line), in the forward report's order. A query's first line is its best hit: lowest E, then
    highest score, then the subject's order in its file."""
    forward = read_report(forward_report).drop_duplicates('qseqid', keep='first')
    reverse = read_report(reverse_report).drop_duplicates('qseqid', keep='first')
    back = dict(zip(reverse['qseqid'], reverse['sseqid']))
    mutual = forward[[back.get(s) == q for q, s in zip(forward['qseqid'], forward['sseqid'])]]
    out = mutual[['qseqid', 'sseqid', 'pident', 'length', 'evalue', 'bitscore']].rename(columns={'qseqid': 'seq1', 'sseqid': 'seq2'})
    return out.reset_index(drop=True)
