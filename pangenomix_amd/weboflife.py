"""Gene content on a species tree and the circular dendrogram (reference weboflife.py). The reference's names, positional
order and defaults:

    get_node_gene_content        one gene: for every node the fraction of the mapped species below it that carry the gene.
                                 The reference's loop restated, quirks included.
    get_node_gene_content_table  NEW: the same for every gene of a gene x species table at once, as a nodes x genes frame
                                 whose column g equals get_node_gene_content for row g of the table value for value. With
                                 ctx=None the sums are numpy rows on the host; with a _native.Context the counts come from
                                 pgx_tree_content (one launch per height of the tree) and only the division is the host's.
    dendrogram_layout            NEW name for the geometry of draw_nx_dendrogram: (depths, angles, node_xy)
    draw_nx_dendrogram           the drawing, on the host: a tree's layout is microseconds of arithmetic

The device path takes regular input only and leaves anything else to the host code unchanged; WEBOFLIFE_PATH_COUNTS says
which path ran. networkx is needed nowhere: a graph is anything with G[node] (the successors, a mapping to the edge's
attributes), iteration, len() and .nodes -- an nx.DiGraph, a PhyloGraph, and for the gene content also an amr.AroGraph.
The two traversals are restated by networkx's rules: bfs_successors and dfs_preorder_nodes in insertion order."""
import collections

import numpy as np
import pandas as pd

try:                                                     # optional: nothing here needs it
    import networkx as _nx
except ImportError:                                      # pragma: no cover
    _nx = None

WEBOFLIFE_PATH_COUNTS = collections.Counter()            # table_device / table_host: per call
_CHUNK_BYTES = 256 << 20                                 # the counts of one device call stay at or under this


class PhyloGraph(object):
    """A directed graph with edge attributes and the few methods this module needs, in the insertion order an nx.DiGraph
    keeps: add_node(), add_edge(u, v, **attributes), G[node], iteration, len(), `in` and .nodes."""

    def __init__(self):
        self._succ = {}

    def add_node(self, node):
        self._succ.setdefault(node, {})

    def add_edge(self, u, v, **attributes):
        self.add_node(u)
        self.add_node(v)
        self._succ[u].setdefault(v, {}).update(attributes)

    def __getitem__(self, node):
        return self._succ[node]

    def __iter__(self):
        return iter(self._succ)

    def __len__(self):
        return len(self._succ)

    def __contains__(self, node):
        try:
            return node in self._succ
        except TypeError:
            return False

    @property
    def nodes(self):
        return list(self._succ)


def _successors(G, node):
    try:
        return G[node]
    except KeyError:
        if _nx is not None:                              # what G.neighbors(root) raises inside bfs_successors
            raise _nx.NetworkXError('The node %s is not in the digraph.' % (node,))
        raise


def __get_bfs_traversal__(G, root):
    ''' Generates a BFS traversal of the graph as a list of nodes, including terminals '''
    # bfs_successors by its rule: parents in first-in-first-out order, each with the successors that were not seen before,
    # in insertion order; a parent without any such successor is left out, the root excepted
    bfs, seen, queue = [], {root}, collections.deque([root])
    _successors(G, root)
    while queue:
        parent = queue.popleft()
        successors = []
        for child in G[parent]:
            if child not in seen:
                seen.add(child)
                successors.append(child)
        if successors or not bfs:
            bfs.append((parent, successors))
        queue.extend(successors)
    node_bfs = [x[0] for x in bfs]                       # sequence of non-terminal nodes, breadth-first
    for node, successors in bfs:                         # appending terminal nodes
        for successor in successors:
            if len(G[successor]) == 0:                   # terminal
                node_bfs.append(successor)
    return node_bfs


def __get_dfs_preorder__(G, root):
    """dfs_preorder_nodes by its rule: a node is listed when it is first reached, successors in insertion order"""
    order, seen, stack = [root], {root}, [iter(_successors(G, root))]
    while stack:
        for child in stack[-1]:
            if child not in seen:
                seen.add(child)
                order.append(child)
                stack.append(iter(G[child]))
                break
        else:
            stack.pop()
    return order


def get_node_gene_content(G, df_gene_pa, mrca_to_species, root='N3623'):
    '''
    Computes the fraction of child species with the gene for nonterminal nodes.
    For terminal nodes, returns 1 if present, 0 otherwise.
    '''
    # The reference's loop as it is. What follows from it: a mapped node is a leaf even where it has children, and the
    # nodes below it still get values of their own; an unmapped childless node divides 0.0 by 0.0 (nan, with numpy's
    # RuntimeWarning); int() truncates, and -1 indexes the last of the two counters.
    node_bfs = __get_bfs_traversal__(G, root)
    node_content = {}
    for node in reversed(node_bfs):
        node_content[node] = np.zeros(2)
        if node in mrca_to_species:
            species = mrca_to_species[node]
            has_gene = df_gene_pa.loc[species]
            node_content[node][int(has_gene)] = 1
        else:
            for child in G[node]:
                node_content[node] += node_content[child]
    for node in node_content:
        presence_rate = float(node_content[node][1]) / node_content[node].sum()
        node_content[node] = presence_rate
    return node_content


# ---- every gene at once --------------------------------------------------------------------------------------------------------
class _GeneTable(object):
    """The rows `genes` (labels; None: all) of a gene x species LightSparseDataFrame or pandas frame: `csr`, the chosen rows
    as float64 with duplicate coordinates summed and stored zeros dropped; `regular`, whether it is a 0/1 table without
    duplicate coordinates."""

    def __init__(self, table, genes):
        import scipy.sparse as sp
        if isinstance(table, pd.DataFrame):
            index, columns = table.index, table.columns
            at = None if genes is None else index.get_indexer(list(genes))
            if at is not None and (at < 0).any():
                raise KeyError(list(genes)[int(np.flatnonzero(at < 0)[0])])
            values = table.to_numpy()
            if values.dtype == object:
                values = values.astype(np.float64)       # (raises for what float() cannot take)
            csr = sp.csr_matrix(values if at is None else values[at])
            duplicates = False
        else:
            index, columns = table.index, table.columns
            at = None if genes is None else np.array([table.index_map[g] for g in genes], dtype=np.int64)
            coo = table.data.tocoo()
            csr = coo.tocsr()                            # (sums duplicate coordinates, as .values does)
            duplicates = csr.nnz != coo.nnz
            if at is not None:
                csr = csr[at]
        self.labels = index if genes is None else list(genes)
        self.csr = csr.astype(np.float64)
        self.csr.eliminate_zeros()
        self.csr.sort_indices()
        self.n_genes, self.n_species = self.csr.shape
        self.column_of = {label: j for j, label in enumerate(columns.tolist() if hasattr(columns, 'tolist') else columns)}
        self.regular = not duplicates and bool((self.csr.data == 1.0).all()) and self.n_species < (1 << 31)
        self._csc = None

    def column(self, species):
        """the values of one species over the chosen genes, dense; KeyError(species) for a species that is no column"""
        j = self.column_of[species]
        if self._csc is None:
            self._csc = self.csr.tocsc()
        lo, hi = self._csc.indptr[j], self._csc.indptr[j + 1]
        col = np.zeros(self.n_genes)
        col[self._csc.indices[lo:hi]] = self._csc.data[lo:hi]
        return col

    def records(self, lo, hi):
        """(rows - lo, species) int32 of the ones of the chosen genes lo .. hi - 1"""
        a, b = self.csr.indptr[lo], self.csr.indptr[hi]
        rows = np.repeat(np.arange(hi - lo, dtype=np.int32), np.diff(self.csr.indptr[lo:hi + 1]))
        return rows, self.csr.indices[a:b].astype(np.int32)


def _presence(col):
    """what `counters[int(value)] = 1` makes of a column of values: the second of two counters is set for 1 and -1, the
    first for 0 and -2 (int() truncates), and anything else raises what int() or the index raises"""
    k = np.trunc(col)
    bad = ~((k >= -2) & (k <= 1))                        # (a NaN fails both comparisons)
    if bad.any():
        value = col[int(np.flatnonzero(bad)[0])]
        if np.isnan(value):
            raise ValueError('cannot convert float NaN to integer')
        if np.isinf(value):
            raise OverflowError('cannot convert float infinity to integer')
        raise IndexError('index %d is out of bounds for axis 0 with size 2' % int(value))
    return (k == 1) | (k == -1)


def _table_host(G, nodes, mrca_to_species, table):
    """the loop of get_node_gene_content with a row of genes where it has one gene; the total of a node is the same for
    every gene, so it is one number per node"""
    out = np.zeros((len(nodes), table.n_genes))
    totals = np.zeros(len(nodes))
    at = {}
    for i, node in enumerate(nodes):
        at[node] = i                                     # (before the children are read, as the reference's np.zeros(2))
        if node in mrca_to_species:
            species = mrca_to_species[node]
            out[i] = _presence(table.column(species))
            totals[i] = 1
        else:
            for child in G[node]:
                j = at[child]                            # KeyError(child): a child that has no value yet
                out[i] += out[j]
                totals[i] += totals[j]
    with np.errstate(invalid='ignore'):                  # 0 / 0 is nan, as in the reference, without its warning
        out /= totals[:, None]
    return out


def _device_plan(G, nodes, mrca_to_species, table):
    """The arrays of pgx_tree_content for the nodes numbered in the order of `nodes` (children come before parents), or
    None for input the host has to take: a table that is not 0/1, a node or species that cannot be hashed, a mapped species
    that is no column, a child without a number or with a number that is not lower (a cycle, a node the traversal left
    out), a node with two parents."""
    if not table.regular:
        return None
    n = len(nodes)
    leaf = np.full(n, -1, dtype=np.int32)
    height = np.zeros(n, dtype=np.int64)
    child_off = np.zeros(n + 1, dtype=np.uint32)
    child, has_parent = [], bytearray(n)
    try:
        number = {node: i for i, node in enumerate(nodes)}
        for i, node in enumerate(nodes):
            if node in mrca_to_species:                  # a leaf: its children are not consulted, and not listed
                j = table.column_of.get(mrca_to_species[node])
                if j is None:
                    return None
                leaf[i] = j
            else:
                for c in G[node]:
                    k = number.get(c)
                    if k is None or k >= i or has_parent[k]:
                        return None
                    has_parent[k] = 1
                    child.append(k)
                    height[i] = max(height[i], height[k] + 1)
            child_off[i + 1] = len(child)
    except TypeError:
        return None
    order = np.argsort(height, kind='stable').astype(np.uint32)
    level_off = np.searchsorted(height[order], np.arange(int(height.max()) + 2)).astype(np.uint32)
    return leaf, child_off, np.array(child, dtype=np.uint32), order, level_off


def _chunk_genes(n_nodes):
    """genes per device call: the most whose counts (rows padded to a multiple of 4) fit _CHUNK_BYTES, at least 1"""
    fit = _CHUNK_BYTES // (4 * n_nodes)
    return int(fit // 4 * 4 if fit >= 4 else max(fit, 1))


def _table_device(ctx, plan, table, n_nodes):
    leaf, child_off, child, order, level_off = plan
    step = _chunk_genes(n_nodes)
    if ctx.tree_content_workspace_bytes(n_nodes, min(step, max(table.n_genes, 1)), child.size) == 0:
        return None                                      # sizes the library refuses
    out = np.empty((n_nodes, table.n_genes))
    totals = None
    stride = lambda n: (n + 3) // 4 * 4                  # noqa: E731  (pgx_tree_content_stride)
    buffer = np.empty(n_nodes * stride(min(step, table.n_genes)), dtype=np.uint32)   # one for every chunk: faulted in once
    for lo in range(0, table.n_genes, step):
        hi = min(lo + step, table.n_genes)
        rows, species = table.records(lo, hi)
        got = ctx.tree_content(rows, species, hi - lo, table.n_species, leaf, child_off, child, order, level_off,
                               return_totals=totals is None,
                               counts=buffer[:n_nodes * stride(hi - lo)].reshape(n_nodes, stride(hi - lo)))
        if got[-1]:
            raise RuntimeError('duplicate coordinates in a table that was checked for them')
        if totals is None:
            totals = got[1][:, None]                     # (the same for every chunk: they do not depend on the genes)
        # both operands are exact integers: the same IEEE division as the host's, on half the bytes
        with np.errstate(invalid='ignore'):
            np.divide(got[0][:, :hi - lo], totals, out=out[:, lo:hi])
    return out


def get_node_gene_content_table(G, df_genes_pa, mrca_to_species, root='N3623', genes=None, ctx=None):
    """get_node_gene_content for every gene at once. df_genes_pa: a gene x species LightSparseDataFrame or pandas frame of
    0 / 1 / bool; genes: the rows to take, by label (None: all, in the table's order). Returns a float64 frame, one row
    per node in the order of get_node_gene_content's dict and one column per gene; column g holds what
    get_node_gene_content(G, <row g as a series>, mrca_to_species, root) returns, nan included, and no warning is emitted.
    ctx: a _native.Context for the device path (regular input only, see the module's text), None for the host's."""
    nodes = __get_bfs_traversal__(G, root)[::-1]
    table = _GeneTable(df_genes_pa, genes)
    values = None
    if ctx is not None:
        plan = _device_plan(G, nodes, mrca_to_species, table)
        if plan is not None:
            values = _table_device(ctx, plan, table, len(nodes))
    WEBOFLIFE_PATH_COUNTS['table_host' if values is None else 'table_device'] += 1
    if values is None:
        values = _table_host(G, nodes, mrca_to_species, table)
    return pd.DataFrame(values, index=pd.Index(nodes, tupleize_cols=False), columns=table.labels, copy=False)


# ---- the dendrogram ------------------------------------------------------------------------------------------------------------
def dendrogram_layout(G, root, length_attr='len'):
    """(depths, angles, node_xy) of draw_nx_dendrogram: the radius of every node (the branch lengths from the root, rounded
    to 8 digits at every step), its angle as {'mean', 'max', 'min'} (terminals evenly spaced in depth-first order, any other
    node over the means of its children) and the positions of the nodes in the order of iteration over G."""
    ''' Compute depths/radius of each node '''
    node_bfs = __get_bfs_traversal__(G, root)
    depths = {root: 0.0}
    for node in node_bfs:
        for child in G[node]:
            child_depth = depths[node] + G[node][child][length_attr]
            depths[child] = round(child_depth, 8)

    ''' Generate terminal node order with depth-first search '''
    dfs = __get_dfs_preorder__(G, root)
    terminal_order = [node for node in dfs if len(G[node]) == 0]
    terminal_set = set(terminal_order)
    n_terminals = len(terminal_set)
    terminal_index = {}                                  # what terminal_order.index(node) gives, without its search
    for i, node in enumerate(terminal_order):
        terminal_index.setdefault(node, i)

    ''' Compute node angles '''
    angles = {}
    terminal_angles = np.arange(0, 1.0, 1.0 / n_terminals) * 2 * np.pi
    for node in reversed(node_bfs):
        if node in terminal_set:   # terminal node, evenly spaced in order previously calculated
            angle = terminal_angles[terminal_index[node]]
            angles[node] = {'mean': angle, 'max': angle, 'min': angle}
        else:   # intermediate node, take average of immediate children
            # (the reference would call a get_angles it never defines for a child without an angle; in a tree there is
            # none, since children come before their parents in the reversed traversal)
            child_angles = [angles[child]['mean'] for child in G[node]]
            angles[node] = {'mean': np.mean(child_angles), 'max': np.max(child_angles), 'min': np.min(child_angles)}

    ''' Compute node final positions '''
    node_xy = np.zeros((len(G), 2))
    for i, node in enumerate(G):
        node_xy[i][0] = depths[node] * np.cos(angles[node]['mean'])
        node_xy[i][1] = depths[node] * np.sin(angles[node]['mean'])
    return depths, angles, node_xy


def draw_nx_dendrogram(G, root, node_colors=None, ax=None, length_attr='len', return_coords=False):
    '''
    Generates a circular dendrogram from a networkx defined phylogeny.

    Parameters
    ----------
    G : nx.DiGraph
        Graph with edges going root -> terminals
    root : str
        Name of node to treet as root
    node_colors : dict, color, or None
        If dict, maps node names to colors. If None, all nodes are black.
        Otherwise, assigns the values to all nodes (default None)
    ax : AxesSubplot
        Subplot to plot onto (default None)
    length_attr : str
        Name of attribute to use to extract edge lengths (default 'len')
    return_coords : bool
        If True, returns both the subplot and node coordinates (default False)
    '''
    import matplotlib as mpl
    import matplotlib.patches
    import matplotlib.pyplot as plt
    connector_color = 'black'
    default_node_color = 'black'
    whitespace_scaling = 1.05
    node_size = 30

    depths, angles, node_xy = dendrogram_layout(G, root, length_attr)
    node_bfs = __get_bfs_traversal__(G, root)
    if type(node_colors) == dict:   # individually defined colors
        node_color_order = [node_colors[node] for node in G.nodes]
    elif node_colors is None:   # if nothing, default black
        node_color_order = [default_node_color] * len(G.nodes)
    else:   # otherwise, pass directly to each node
        node_color_order = [node_colors] * len(G.nodes)

    ''' Generate connecting lines '''
    if ax is None:
        fig, ax = plt.subplots(1, 1)
    for parent in node_bfs:
        if len(G[parent]) > 0:   # non-terminal
            ''' Draw arcs'''
            diameter = 2.0 * depths[parent]
            arc = mpl.patches.Arc(xy=(0, 0), width=diameter, height=diameter,
                                  theta1=angles[parent]['min'] * 180.0 / np.pi,
                                  theta2=angles[parent]['max'] * 180.0 / np.pi,
                                  linewidth=1, fill=False, color=connector_color)
            ax.add_patch(arc)

            ''' Draw child branches '''
            for child in G[parent]:
                x1 = depths[child] * np.cos(angles[child]['mean'])
                y1 = depths[child] * np.sin(angles[child]['mean'])
                x2 = depths[parent] * np.cos(angles[child]['mean'])
                y2 = depths[parent] * np.sin(angles[child]['mean'])
                ax.plot([x1, x2], [y1, y2], color=connector_color)

    ''' Draw nodes, formatting '''
    ax.scatter(node_xy[:, 0], node_xy[:, 1], s=node_size, c=node_color_order, zorder=10)
    max_radius = max(depths.values())
    ax.set_xlim([-whitespace_scaling * max_radius, whitespace_scaling * max_radius])
    ax.set_ylim([-whitespace_scaling * max_radius, whitespace_scaling * max_radius])
    if return_coords:
        return ax, node_xy
    return ax
