"""The definition of pgx_graph_reach in plain Python (include/pgx.h "Shortest-path lengths"): one breadth-first search per
(source, target), nothing shared between them."""
import collections

import numpy as np


def csr(n_nodes, edges):
    """(succ_off uint32 [n_nodes + 1], succ uint32) of the directed edges (u, v), in the order given per node"""
    lists = [[] for _ in range(n_nodes)]
    for u, v in edges:
        lists[u].append(v)
    off = np.zeros(n_nodes + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(x) for x in lists])
    succ = np.array([v for x in lists for v in x], dtype=np.uint32)
    return off, succ


def path_nodes(succ_off, succ, s, t):
    """the number of nodes on a shortest path from s to t, 0 for none"""
    if s == t:
        return 1
    seen, queue = {s}, collections.deque([(s, 1)])
    while queue:
        v, d = queue.popleft()
        for w in succ[succ_off[v]:succ_off[v + 1]].tolist():
            if w == t:
                return d + 1
            if w not in seen:
                seen.add(w)
                queue.append((w, d + 1))
    return 0


def lengths(succ_off, succ, targets, sources):
    out = np.zeros((len(sources), len(targets)), dtype=np.uint32)
    for i, s in enumerate(sources):
        for j, t in enumerate(targets):
            out[i, j] = path_nodes(succ_off, succ, int(s), int(t))
    return out


def rounds(succ_off, succ, targets):
    """1 + the most edges on a shortest path from any node to a target it reaches"""
    n = len(succ_off) - 1
    if n == 0:
        return 0
    pred = [[] for _ in range(n)]
    for v in range(n):
        for w in succ[succ_off[v]:succ_off[v + 1]].tolist():
            pred[w].append(v)
    most = 0
    for t in set(int(x) for x in targets):                 # a search backwards from the target: levels = edges to it
        level, frontier = {t: 0}, [t]
        while frontier:
            nxt = []
            for w in frontier:
                for v in pred[w]:
                    if v not in level:
                        level[v] = level[w] + 1
                        nxt.append(v)
            frontier = nxt
        most = max(most, max(level.values()))
    return most + 1
