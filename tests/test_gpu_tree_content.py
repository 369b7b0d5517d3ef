"""The gene content of tree nodes on the device (csrc/tree.hip; include/pgx.h "Gene content of tree nodes")
against the contract in plain Python (tests/tree_content_model.py). Counts and totals are integers: equal, not close. The
shapes are the smallest at which each part can go wrong: lane groups of 4 genes, the edges of a 64-bit word, the stride pad,
more children than a wave has lanes or the unrolled loop takes at once, many levels, every kind of node."""
import numpy as np
import pytest

import dev_entry_checks as dev
import tree_content_model as model
from pangenomix_amd import _native, synth

pytestmark = pytest.mark.gpu

GENES = (1, 3, 4, 5, 63, 64, 65, 257)
SPECIES = (1, 2, 65)
INVALID = -1                                              # PGX_ERR_INVALID


# ---- trees: (leaf_species, one list of children per node); a mapped node i takes species i % n_species ---------------------
def mapped(nodes, n, n_species):
    leaf = np.full(n, -1, dtype=np.int32)
    for i in nodes:
        leaf[i] = i % n_species
    return leaf


def quirks(n_species):
    """0 -> 1, 2, 3 (a polytomy); 1 is MAPPED and has the subtree 4 -> 5, 6 below it; 2 -> 7, 8 (8 an unmapped leaf), 9;
    3 -> 10, 11, 12, 13, 14 (five children: one round of the unrolled loop and a rest); 10 and 10 + n_species share a
    species where there are few"""
    children = [[1, 2, 3], [4], [7, 8, 9], [10, 11, 12, 13, 14], [5, 6]] + [[] for _ in range(10)]
    leaf = mapped([1, 5, 6, 7, 9, 10, 11, 12, 13, 14], 15, n_species)
    leaf[14] = leaf[7]                                     # two nodes on one species, whatever n_species is
    return leaf, children


def single(n_species, is_mapped):
    return mapped([0] if is_mapped else [], 1, n_species), [[]]


def star(n_species, n=300):
    return mapped(range(1, n + 1), n + 1, n_species), [list(range(1, n + 1))] + [[] for _ in range(n)]


def caterpillar(n_species, height=70):
    """inner node 2k has the leaf 2k + 1 and the next inner node 2k + 2; the last inner node has two leaves"""
    n = 2 * height + 1
    children = [[] for _ in range(n)]
    for k in range(height):
        children[2 * k] = [2 * k + 1, 2 * k + 2]
    leaf = mapped([2 * k + 1 for k in range(height)] + [n - 1], n, n_species)
    return leaf, children


def balanced(n_species, leaves=128):
    n = 2 * leaves - 1
    children = [[2 * i + 1, 2 * i + 2] if 2 * i + 2 < n else [] for i in range(n)]
    return mapped(range(leaves - 1, n), n, n_species), children


TREES = {'quirks': quirks, 'mapped single': lambda s: single(s, True), 'unmapped single': lambda s: single(s, False),
         'star': star, 'caterpillar': caterpillar, 'balanced': balanced}


def table(n_genes, n_species, seed):
    rng = np.random.default_rng(seed)
    present = rng.random((n_genes, n_species)) < rng.random((n_genes, 1))
    present[-1, :] = True                                  # the last gene, next to the pad, everywhere
    return present


def arrays(leaf, children):
    child_off, child = model.csr(children)
    order, level_off = model.levels(leaf, child_off, child)
    return leaf, child_off, child, order, level_off


def check(ctx, present, leaf, children):
    n_genes, n_species = present.shape
    tree = arrays(leaf, children)
    rows, species = np.nonzero(present)
    counts, totals, dup = ctx.tree_content(rows, species, n_genes, n_species, *tree, return_totals=True)
    want_counts, want_totals = model.tree_content(present, *tree[:3])
    assert dup == 0 and counts.dtype == np.uint32 and counts.shape == (len(leaf), model.stride(n_genes)) == want_counts.shape
    assert np.array_equal(counts, want_counts)             # the pad entries too: zeros
    assert not counts[:, n_genes:].any()
    assert np.array_equal(totals, want_totals)
    alone, dup = ctx.tree_content(rows, species, n_genes, n_species, *tree)       # out_totals NULL
    assert dup == 0 and alone.tobytes() == counts.tobytes()
    again = ctx.tree_content(rows, species, n_genes, n_species, *tree, return_totals=True)
    assert again[0].tobytes() == counts.tobytes() and again[1].tobytes() == totals.tobytes()
    kept = np.full(counts.shape, 0x6E6E6E6E, dtype=np.uint32)         # the caller's buffer: every entry written, the pad too
    into = ctx.tree_content(rows, species, n_genes, n_species, *tree, counts=kept)
    assert into[0] is kept and kept.tobytes() == counts.tobytes()
    with pytest.raises(ValueError):
        ctx.tree_content(rows, species, n_genes, n_species, *tree, counts=np.zeros((len(leaf), counts.shape[1] + 4), dtype=np.uint32))
    return counts, totals


@pytest.mark.parametrize('n_species', SPECIES)
@pytest.mark.parametrize('n_genes', GENES)
def test_every_gene_count_and_word_edge(n_genes, n_species, gpu_ctx):
    assert gpu_ctx.tree_content_stride(n_genes) == model.stride(n_genes)
    leaf, children = quirks(n_species)
    counts, totals = check(gpu_ctx, table(n_genes, n_species, n_genes * 100 + n_species), leaf, children)
    assert totals.tolist() == [8, 1, 2, 5, 2, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1]
    assert counts[0, n_genes - 1] == 8 and not counts[8].any()           # the gene that is everywhere; the unmapped leaf
    assert counts[1].max() <= 1 and counts[4].max() <= 2                 # the mapped inner node is a leaf; its subtree has values


@pytest.mark.parametrize('shape', ((65, 65), (257, 2)))
@pytest.mark.parametrize('name', sorted(TREES))
def test_every_kind_of_tree(name, shape, gpu_ctx):
    leaf, children = TREES[name](shape[1])
    counts, totals = check(gpu_ctx, table(shape[0], shape[1], len(leaf)), leaf, children)
    if name == 'caterpillar':
        assert arrays(leaf, children)[4].size == 72 and totals[0] == 71  # 71 heights
    if name == 'unmapped single':
        assert totals.tolist() == [0] and not counts.any()
    if shape[1] == 65 and name == 'quirks':
        assert len(set(leaf[leaf >= 0].tolist())) < 65                    # species that no node maps


def test_a_generated_phylogeny(gpu_ctx):
    G, root, m, tab = synth.phylogeny(500, 7, n_genes=1000, max_children=6, mapped_internal=25, unmapped_leaves=30, unused_species=9)
    nodes = list(G)
    number = {node: i for i, node in enumerate(nodes)}
    column = tab.column_map
    leaf = np.array([column[m[node]] if node in m else -1 for node in nodes], dtype=np.int32)
    children = [[number[c] for c in G[node]] for node in nodes]
    counts, totals = check(gpu_ctx, tab.values.astype(bool), leaf, children)
    assert len(nodes) > 700 and int(totals[number[root]]) < 500 + 25 and totals.max() == totals[number[root]]


def test_invalid_calls_are_refused_before_anything_is_launched(gpu_ctx):
    lib, P, h = _native.lib(), _native._ptr, gpu_ctx._h
    present = table(6, 3, 1)
    rows, species = (a.astype(np.int32) for a in np.nonzero(present))
    good_leaf = np.array([-1, -1, 0, 1, 2], dtype=np.int32)
    good_children = [[1, 2], [3, 4], [], [], []]
    counts = np.full((5, 8), 0x6E6E6E6E, dtype=np.uint32)
    totals = np.full(5, 0x6E6E6E6E, dtype=np.uint32)

    def call(leaf=good_leaf, children=good_children, order=None, level_off=None, n_nodes=5, n_genes=6):
        child_off, child = model.csr(children)
        want_order, want_off = model.levels(good_leaf, *model.csr(good_children))
        order = want_order if order is None else np.array(order, dtype=np.uint32)
        level_off = want_off if level_off is None else np.array(level_off, dtype=np.uint32)
        return lib.pgx_tree_content(h, P(rows), P(species), rows.size, n_genes, 3, P(leaf), P(child_off), P(child), n_nodes,
                                    P(order), P(level_off), level_off.size - 1, P(counts), P(totals), None)
    assert model.levels(good_leaf, *model.csr(good_children))[1].tolist() == [0, 3, 4, 5]
    gpu_ctx.profile(True)
    gpu_ctx.profile_reset()
    try:
        for name, kwargs in (('a child on an equal level', dict(order=[2, 3, 4, 1, 0], level_off=[0, 3, 5])),
                             ('a node twice in order', dict(order=[2, 3, 4, 1, 1])),
                             ('a node with two parents', dict(children=[[1, 2, 3], [3, 4], [], [], []])),
                             ('a species that does not exist', dict(leaf=np.array([-1, -1, 0, 1, 3], dtype=np.int32))),
                             ('a species below -1', dict(leaf=np.array([-1, -1, 0, 1, -2], dtype=np.int32))),
                             ('a mapped node above height 0', dict(leaf=np.array([-1, 0, 0, 1, 2], dtype=np.int32))),
                             ('level offsets that stop short', dict(level_off=[0, 3, 4, 4])),
                             ('more than 2^31 entries', dict(n_nodes=1 << 20, n_genes=(1 << 11) + 1))):
            assert call(**kwargs) == INVALID, name
            assert lib.pgx_last_error().decode().startswith('tree_'), name     # a message of this call
            assert (counts == 0x6E6E6E6E).all() and (totals == 0x6E6E6E6E).all(), name
        assert not any(k.startswith('tree_') for k in gpu_ctx.profile_read())
        assert call() == 0 and not (counts == 0x6E6E6E6E).any()
        launched = gpu_ctx.profile_read()
        assert launched['tree_leaf_kernel'][1] == 1 and launched['tree_sum_kernel'][1] == 2
    finally:
        gpu_ctx.profile(False)
    assert gpu_ctx.tree_content_workspace_bytes(1 << 20, 1 << 11, 0) > 0           # exactly 2^31 entries
    assert gpu_ctx.tree_content_workspace_bytes(1 << 20, (1 << 11) + 1, 0) == 0
    assert gpu_ctx.tree_content_workspace_bytes(5, 6, 1 << 31) > 0 and gpu_ctx.tree_content_workspace_bytes(5, 6, (1 << 31) + 1) == 0
    g = dev.guarded(4096, 0x5A)
    for n_nodes, n_genes, n_edges in ((1 << 20, (1 << 11) + 1, 4), (5, 6, (1 << 31) + 1)):
        with pytest.raises(_native.PgxError) as e:
            gpu_ctx.tree_content_dev(g.ptr, n_genes, 3, g.ptr, g.ptr, g.ptr, n_nodes, n_edges, g.ptr, [0, n_nodes], g.ptr, g.ptr,
                                     g.ptr, 256)
        assert e.value.status == INVALID
    assert g.is_still_garbage()
    g.assert_guards_intact()


# ---- the device entry ------------------------------------------------------------------------------------------------------
def dev_case(ctx, name, n_genes, n_species):
    leaf, children = TREES[name](n_species)
    present = table(n_genes, n_species, 11)
    tree = arrays(leaf, children)
    rows, species = np.nonzero(present)
    bits = ctx.presence_bitmap(rows, species, n_genes, n_species)
    return present, tree, bits


def run_dev(ctx, present, tree, bits, fill, stream, with_totals=True):
    leaf, child_off, child, order, level_off = tree
    n_genes, n_species = present.shape
    n = leaf.size
    ws_bytes = ctx.tree_content_workspace_bytes(n, n_genes, child.size)
    assert ws_bytes > 0
    with dev.stream_scope(stream) as handle:
        d = [dev.upload(a) for a in (bits, leaf, child_off, child, order)]
        counts, totals, ws = dev.guarded(4 * n * model.stride(n_genes), fill), dev.guarded(4 * n, fill), dev.guarded(ws_bytes, fill)
        with dev.unchanged(*(x for x in d if x.nbytes)):
            ctx.tree_content_dev(d[0].ptr, n_genes, n_species, d[1].ptr, d[2].ptr, d[3].ptr, n, child.size, d[4].ptr, level_off,
                                 counts.ptr, totals.ptr if with_totals else None, ws.ptr, ws_bytes, handle)
    for x in (counts, totals, ws):
        x.assert_guards_intact()
    assert with_totals or totals.is_still_garbage()
    return counts.numpy(np.uint32).reshape(n, -1), totals.numpy(np.uint32)


@pytest.mark.parametrize('name,n_genes,n_species', (('quirks', 65, 2), ('star', 257, 65), ('caterpillar', 5, 3)))
@pytest.mark.parametrize('stream', dev.STREAMS)
def test_device_entry_on_caller_tensors(stream, name, n_genes, n_species, gpu_ctx):
    present, tree, bits = dev_case(gpu_ctx, name, n_genes, n_species)
    want = model.tree_content(present, *tree[:3])
    per_fill = []
    for fill in dev.FILLS:
        got = run_dev(gpu_ctx, present, tree, bits, fill, stream)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        per_fill.append(got)
    dev.same_bytes(per_fill)
    alone = run_dev(gpu_ctx, present, tree, bits, 0xFF, stream, with_totals=False)
    assert np.array_equal(alone[0], want[0])


def test_device_entry_does_not_allocate(gpu_ctx):
    import torch
    present, tree, bits = dev_case(gpu_ctx, 'balanced', 257, 65)
    leaf, child_off, child, order, level_off = tree
    n = leaf.size
    d = [dev.upload(a) for a in (bits, leaf, child_off, child, order)]
    counts, totals, ws = dev.guarded(4 * n * model.stride(257), 0xFF), dev.guarded(4 * n, 0xFF), dev.guarded(256, 0xFF)
    dev.assert_no_allocation(lambda: gpu_ctx.tree_content_dev(d[0].ptr, 257, 65, d[1].ptr, d[2].ptr, d[3].ptr, n, child.size, d[4].ptr,
                                                              level_off, counts.ptr, totals.ptr, ws.ptr, 256))
    torch.cuda.synchronize()
    want = model.tree_content(present, *tree[:3])
    assert np.array_equal(counts.numpy(np.uint32).reshape(n, -1), want[0]) and np.array_equal(totals.numpy(np.uint32), want[1])
