"""TEST INFRASTRUCTURE: the contract of pgx_tree_content (include/pgx.h, "Gene content of tree nodes") in plain Python, the
trees the GPU tests run it on, and a stand-in for _native.Context that answers tree_content from the model."""
import numpy as np


def stride(n_genes):
    return (int(n_genes) + 3) // 4 * 4


def levels(leaf_species, child_off, child):
    """(order, level_off) by the rule: height 0 for a mapped node and for a childless unmapped one, else 1 + the largest
    height among the children. Nodes of one height keep their numbers' order."""
    n = len(leaf_species)
    height = [-1] * n
    for root in range(n):
        stack = [root]
        while stack:
            v = stack[-1]
            kids = [] if leaf_species[v] >= 0 else [int(c) for c in child[child_off[v]:child_off[v + 1]]]
            todo = [c for c in kids if height[c] < 0]
            if todo:
                stack.extend(todo)
                continue
            height[v] = 1 + max(height[c] for c in kids) if kids else 0
            stack.pop()
    height = np.array(height, dtype=np.int64)
    order = np.argsort(height, kind='stable').astype(np.uint32)
    level_off = np.searchsorted(height[order], np.arange(int(height.max()) + 2 if n else 1)).astype(np.uint32)
    return order, level_off


def check_tree(leaf_species, child_off, child, order, level_off, n_species):
    """raises ValueError naming the rule of the host entry that is broken"""
    n = len(leaf_species)
    if sorted(int(v) for v in order) != list(range(n)):
        raise ValueError('every node once in order')
    if level_off[0] != 0 or level_off[-1] != n or (np.diff(np.asarray(level_off, dtype=np.int64)) < 0).any():
        raise ValueError('level_off from 0 to n_nodes')
    level_of = np.zeros(n, dtype=np.int64)
    for h in range(len(level_off) - 1):
        level_of[np.asarray(order[level_off[h]:level_off[h + 1]], dtype=np.int64)] = h
    parents = np.zeros(n, dtype=np.int64)
    for v in range(n):
        if not -1 <= leaf_species[v] < n_species:
            raise ValueError('leaf_species below n_species')
        kids = [int(c) for c in child[child_off[v]:child_off[v + 1]]]
        if leaf_species[v] >= 0 and level_of[v] != 0:
            raise ValueError('a mapped node at height 0')
        if leaf_species[v] < 0 and kids and level_of[v] == 0:
            raise ValueError('an unmapped node with children above height 0')
        for c in kids:
            parents[c] += 1
            if leaf_species[v] < 0 and level_of[c] >= level_of[v]:
                raise ValueError('a child at a strictly lower level')
    if (parents > 1).any():
        raise ValueError('no node is a child of two nodes')


def tree_content(present, leaf_species, child_off, child):
    """present: bool [n_genes, n_species]. (counts uint32 [n_nodes, stride], totals uint32 [n_nodes]) by the three rules."""
    n_genes = present.shape[0]
    n = len(leaf_species)
    counts = np.zeros((n, stride(n_genes)), dtype=np.uint32)
    totals = np.zeros(n, dtype=np.uint32)
    order, _ = levels(leaf_species, child_off, child)
    for v in order.tolist():
        if leaf_species[v] >= 0:
            counts[v, :n_genes] = present[:, leaf_species[v]]
            totals[v] = 1
        else:
            for c in child[child_off[v]:child_off[v + 1]]:
                counts[v] += counts[int(c)]
                totals[v] += totals[int(c)]
    return counts, totals


def dense(rows, species, n_genes, n_species):
    present = np.zeros((n_genes, n_species), dtype=bool)
    present[np.asarray(rows, dtype=np.int64), np.asarray(species, dtype=np.int64)] = True
    return present


def csr(children):
    """children: one list per node -> (child_off, child)"""
    child_off = np.zeros(len(children) + 1, dtype=np.uint32)
    child_off[1:] = np.cumsum([len(c) for c in children])
    return child_off, np.array([x for c in children for x in c], dtype=np.uint32)


class StandIn(object):
    """what weboflife asks of a _native.Context; every call is checked against the rules of the host entry"""

    def __init__(self):
        self.calls = []

    def tree_content_workspace_bytes(self, n_nodes, n_genes, n_edges):
        return 256 if n_nodes * stride(n_genes) <= 1 << 31 and n_edges <= 1 << 31 else 0

    def tree_content(self, rows, species, n_genes, n_species, leaf_species, child_off, child, order, level_off,
                     return_totals=False, counts=None):
        for a, t in ((rows, np.int32), (species, np.int32), (leaf_species, np.int32), (child_off, np.uint32), (child, np.uint32),
                     (order, np.uint32), (level_off, np.uint32)):
            assert a.dtype == t and a.ndim == 1
        check_tree(leaf_species, child_off, child, order, level_off, n_species)
        want_order, want_off = levels(leaf_species, child_off, child)
        assert level_off.tolist() == want_off.tolist()
        for h in range(len(want_off) - 1):                # the same nodes at every height
            assert sorted(order[level_off[h]:level_off[h + 1]].tolist()) == sorted(want_order[want_off[h]:want_off[h + 1]].tolist())
        assert rows.size == 0 or (0 <= rows.min() and rows.max() < n_genes and 0 <= species.min() and species.max() < n_species)
        coords = set(zip(rows.tolist(), species.tolist()))
        want, totals = tree_content(dense(rows, species, n_genes, n_species), leaf_species, child_off, child)
        if counts is None:
            counts = want
        else:                                             # the caller's buffer, as the binding fills it
            assert counts.dtype == np.uint32 and counts.shape == want.shape and counts.flags.c_contiguous
            counts[...] = want
        self.calls.append((n_genes, len(leaf_species)))
        dup = rows.size - len(coords)
        return (counts, totals, dup) if return_totals else (counts, dup)
