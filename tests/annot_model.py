"""A plain-Python model of pgx_annot_vote, straight from the definition in include/pgx.h ("Ordered de-duplication of rows of
ids and the plurality vote of runs of rows"), and the builders of the row and run sets the GPU tests put through it. Nothing
here is clever on purpose: lists, tuples, and a count per row."""
import numpy as np


def vote(rows, run_off):
    """rows: a list of lists of ids >= 0; run_off: n_runs + 1 offsets into it. Returns (keep, winner, votes, differs) as
    Context.annot_vote does."""
    keep, lists = [], []
    for row in rows:
        kept = []
        for p, x in enumerate(row):
            first = x not in row[:p]
            keep.append(1 if first else 0)
            if first:
                kept.append(x)
        lists.append(tuple(kept))
    n_runs = len(run_off) - 1
    winner, votes, differs = [], [], [0] * len(rows)
    for u in range(n_runs):
        members = range(int(run_off[u]), int(run_off[u + 1]))
        count = {r: sum(1 for q in members if lists[q] == lists[r]) for r in members}
        best = max(count.values())
        w = min(r for r in members if count[r] == best)
        winner.append(w)
        votes.append(best)
        for r in members:
            differs[r] = 1 if lists[r] != lists[w] else 0
    return (np.array(keep, dtype=np.uint8), np.array(winner, dtype=np.int32), np.array(votes, dtype=np.uint32),
            np.array(differs, dtype=np.uint8))


def vote_fast(rows, run_off):
    """The same result for runs of thousands of rows: a dictionary per run in place of the quadratic count. Checked against
    vote() in tests/test_annotations_host.py."""
    keep, lists = [], []
    for row in rows:
        seen, kept = set(), []
        for x in row:
            keep.append(0 if x in seen else 1)
            if x not in seen:
                seen.add(x)
                kept.append(x)
        lists.append(tuple(kept))
    winner, votes, differs = [], [], [0] * len(rows)
    for u in range(len(run_off) - 1):
        lo, hi = int(run_off[u]), int(run_off[u + 1])
        count, first = {}, {}
        for r in range(lo, hi):
            count[lists[r]] = count.get(lists[r], 0) + 1
            first.setdefault(lists[r], r)
        best = max(count.values())
        w = min(first[k] for k in count if count[k] == best)
        winner.append(w)
        votes.append(best)
        for r in range(lo, hi):
            differs[r] = 1 if lists[r] != lists[w] else 0
    return (np.array(keep, dtype=np.uint8), np.array(winner, dtype=np.int32), np.array(votes, dtype=np.uint32),
            np.array(differs, dtype=np.uint8))


def flatten(rows):
    """(tok int32, row_off uint64) of a list of rows"""
    row_off = np.zeros(len(rows) + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in rows], out=row_off[1:])
    tok = np.array([x for r in rows for x in r], dtype=np.int32)
    return tok, row_off


def row_shapes(length, rng):
    """rows of one length: all distinct, all equal, a repeat of the first id at the end, of the last id at the start,
    random with repeats -- each where the length allows it"""
    base = [int(x) for x in rng.permutation(max(length, 1) * 3)[:length] + 7]
    rows = [list(base)]
    if length >= 1:
        rows.append([base[0]] * length)
        rows.append([int(x) for x in rng.integers(0, max(length // 3, 1), length)])
    if length >= 2:
        rows.append(base[:-1] + [base[0]])                  # the last position repeats the first
        rows.append([base[-1]] + base[1:])                  # the first position holds what the last repeats
        rows.append([base[0], base[0]] + base[2:])
    return rows


def run_of(size, kind, rng, length=3):
    """a run of `size` rows: 'equal', 'distinct', 'tie' (two lists with the same count, the first-seen must win; its rows do
    not come first), 'mixed' (a few lists, unequal counts, written with and without repeats)"""
    if kind == 'equal':
        return [[5, 9, 5, 2][:length + 1] for _ in range(size)]
    if kind == 'distinct':
        return [[1000 + i, 3] for i in range(size)]
    if kind == 'tie':
        a, b = [4, 8], [8, 4]                               # the same set in another order
        rows = [list(a) if i % 2 == 0 else list(b) for i in range(size - size % 2)]
        if size % 2:
            rows.insert(1, [1 << 20])                       # an odd one that belongs to neither
        if size >= 4:
            rows[0], rows[1] = rows[1], rows[0]             # b is seen first and must win
        return rows
    assert kind == 'mixed'
    pool = [[1, 2], [1, 1, 2], [1, 2, 3], [2, 1], [], [1], [1, 2, 3, 1, 2, 3], [7] * 5]
    return [list(pool[int(i)]) for i in rng.integers(0, len(pool), size)]
