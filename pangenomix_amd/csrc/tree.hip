// Gene content of every node of a rooted tree (reference weboflife.py:16-35 get_node_gene_content: one gene per call, two
// np.zeros(2) per node and one pandas .loc per leaf). Here every gene at once: out_counts[v][g] = how many of the mapped
// nodes at or below v carry gene g, out_totals[v] = how many mapped nodes there are; the quotient is the reference's value.
//
// The tree is child lists (CSR) plus the nodes grouped by height: order[level_off[h] .. level_off[h + 1]) are the nodes of
// height h. Height 0 holds the mapped nodes (leaf_species[v] >= 0: leaves even where they have children, which are not
// consulted) and the childless unmapped ones; every other node lies one above its highest child. A node's row is then the
// sum of rows that an EARLIER launch wrote: one launch per height on one stream, and the order of the launches is the only
// synchronisation there is. No atomics, no LDS, no cross-lane traffic; every sum is an integer sum in the children's CSR
// order, so the same input gives the same bytes on every call.
//
// Kernels (a workgroup works on ONE node, so the tree arrays are uniform across it; lane q owns genes 4q .. 4q + 3, and
// with totals one further lane of the node owns the node's total):
//   tree_leaf_kernel  height 0: the lane reads the one word of the species' bitmap row that holds its four bits (a wave
//                     reads one or two words) and stores one uint4 of 0 / 1, zeros for an unmapped node
//   tree_sum_kernel   height h > 0: the lane walks the node's children, four 16-byte loads of four children's rows in flight
//                     before the adds, and stores 16 bytes
// Rows are pgx_tree_content_stride(n_genes) entries, a multiple of 4, so every access is an aligned 16 bytes; the pad
// entries are written as zeros. Every output row is written once and read once (by its parent's lane): the traffic is
// 2 x n_nodes x stride x 4 bytes, the bitmap words and the tree arrays being small beside it.
// Ids that are not nodes or species are skipped by both kernels (the host entry refuses them; the device entry does not look).
#include "pgx_internal.h"

namespace {

typedef unsigned long long u64;

constexpr int TC_THREADS = 256;
constexpr u64 TC_MAX_ENTRIES = 1ull << 31;                 // n_nodes x stride
constexpr u64 TC_MAX_EDGES = 1ull << 31;
constexpr size_t TC_WS_BYTES = 256;                        // nothing is kept there today; 0 has to mean "refused"

struct TreeGeom {
    uint32_t stride, groups, items, blocks_per_node;       // items: the 4-gene groups, and the total when it is wanted
};

uint32_t tree_stride(uint32_t n_genes) { return (uint32_t)((((u64)n_genes + 3u) / 4u) * 4u); }

bool tree_sizes_ok(uint32_t n_nodes, uint32_t n_genes, u64 n_edges) {
    return (u64)n_nodes * ((((u64)n_genes + 3u) / 4u) * 4u) <= TC_MAX_ENTRIES && n_edges <= TC_MAX_EDGES;
}

TreeGeom tree_geom(uint32_t n_genes, bool totals) {
    TreeGeom g;
    g.stride = tree_stride(n_genes);
    g.groups = g.stride / 4u;
    g.items = g.groups + (totals ? 1u : 0u);
    g.blocks_per_node = (g.items + TC_THREADS - 1u) / TC_THREADS;
    return g;
}

__device__ __forceinline__ uint4 add4(uint4 a, uint4 b) { return make_uint4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ uint4 keep4(uint4 a, bool keep) {
    const uint32_t m = keep ? 0xFFFFFFFFu : 0u;
    return make_uint4(a.x & m, a.y & m, a.z & m, a.w & m);
}

__global__ __launch_bounds__(TC_THREADS) void tree_leaf_kernel(const u64 *__restrict__ bits, uint32_t bit_stride,
                                                               uint32_t n_species, const int32_t *__restrict__ leaf_species,
                                                               const uint32_t *__restrict__ level_nodes, uint32_t n_nodes,
                                                               uint32_t n_genes, TreeGeom geom, uint32_t *__restrict__ counts,
                                                               uint32_t *__restrict__ totals) {
    const uint32_t q = (blockIdx.x % geom.blocks_per_node) * TC_THREADS + threadIdx.x;
    const uint32_t v = level_nodes[blockIdx.x / geom.blocks_per_node];
    if (q >= geom.items || v >= n_nodes) return;
    const int32_t s = leaf_species[v];
    if (q == geom.groups) {                                 // (only with totals: items = groups + 1)
        totals[v] = s >= 0 ? 1u : 0u;
        return;
    }
    const uint32_t g0 = q * 4u;
    uint4 r = make_uint4(0u, 0u, 0u, 0u);
    if (s >= 0 && (uint32_t)s < n_species) {
        // g0 is a multiple of 4: the four bits lie in one word
        const uint32_t w = (uint32_t)(bits[(size_t)s * bit_stride + (g0 >> 6)] >> (g0 & 63u));
        r.x = w & 1u;
        r.y = g0 + 1u < n_genes ? (w >> 1) & 1u : 0u;
        r.z = g0 + 2u < n_genes ? (w >> 2) & 1u : 0u;
        r.w = g0 + 3u < n_genes ? (w >> 3) & 1u : 0u;
    }
    *reinterpret_cast<uint4 *>(counts + (size_t)v * geom.stride + g0) = r;
}

// counts is read (the children's rows) and written (the node's own row): no __restrict__ on it
__global__ __launch_bounds__(TC_THREADS) void tree_sum_kernel(const uint32_t *__restrict__ child_off,
                                                              const uint32_t *__restrict__ child, uint32_t n_edges,
                                                              const uint32_t *__restrict__ level_nodes, uint32_t n_nodes,
                                                              TreeGeom geom, uint32_t *counts, uint32_t *totals) {
    const uint32_t q = (blockIdx.x % geom.blocks_per_node) * TC_THREADS + threadIdx.x;
    const uint32_t v = level_nodes[blockIdx.x / geom.blocks_per_node];
    if (q >= geom.items || v >= n_nodes) return;
    uint32_t begin = child_off[v], end = child_off[v + 1];
    if (begin > n_edges) begin = n_edges;
    if (end > n_edges) end = n_edges;
    if (end < begin) end = begin;
    if (q == geom.groups) {
        uint32_t t = 0;
        for (uint32_t e = begin; e < end; ++e) {
            const uint32_t x = child[e];
            if (x < n_nodes) t += totals[x];
        }
        totals[v] = t;
        return;
    }
    const uint4 *rows = reinterpret_cast<const uint4 *>(counts) + q;      // + x * groups: child x's four entries
    const size_t groups = geom.groups;
    // A child that is no node adds nothing: its load goes to row 0 and is masked out, so that the four loads of a round
    // are unconditional and in flight together (a select between a loaded row and zeros made the compiler branch
    // around every load).
    uint4 acc = make_uint4(0u, 0u, 0u, 0u);
    uint32_t e = begin;
    for (; e + 4u <= end; e += 4u) {
        const uint32_t x0 = child[e], x1 = child[e + 1u], x2 = child[e + 2u], x3 = child[e + 3u];
        const uint4 a = rows[(x0 < n_nodes ? x0 : 0u) * groups];
        const uint4 b = rows[(x1 < n_nodes ? x1 : 0u) * groups];
        const uint4 c = rows[(x2 < n_nodes ? x2 : 0u) * groups];
        const uint4 d = rows[(x3 < n_nodes ? x3 : 0u) * groups];
        acc = add4(acc, add4(add4(keep4(a, x0 < n_nodes), keep4(b, x1 < n_nodes)), add4(keep4(c, x2 < n_nodes), keep4(d, x3 < n_nodes))));
    }
    for (; e < end; ++e) {
        const uint32_t x = child[e];
        acc = add4(acc, keep4(rows[(x < n_nodes ? x : 0u) * groups], x < n_nodes));
    }
    reinterpret_cast<uint4 *>(counts)[v * groups + q] = acc;
}

// ---- launches ------------------------------------------------------------------------------------------------------------
// level_off is the HOST's: it sizes the grids. Everything else is on the device. Only enqueues on `stream`.
int tree_run(pgx_ctx *ctx, const u64 *d_bits, uint32_t n_genes, uint32_t n_species, const int32_t *d_leaf,
             const uint32_t *d_child_off, const uint32_t *d_child, uint32_t n_nodes, uint32_t n_edges, const uint32_t *d_order,
             const uint32_t *level_off, uint32_t n_levels, uint32_t *d_counts, uint32_t *d_totals, hipStream_t stream) {
    const TreeGeom geom = tree_geom(n_genes, d_totals != nullptr);
    if (geom.items == 0) return PGX_OK;                    // no genes and no totals: nothing to write
    for (uint32_t h = 0; h < n_levels; ++h) {
        const uint32_t lo = level_off[h], n_here = level_off[h + 1] - lo;
        if (n_here == 0) continue;
        const u64 blocks = (u64)n_here * geom.blocks_per_node;         // <= n_nodes x stride / 1024 + n_nodes
        if (blocks >= (1ull << 31)) {
            pgx_set_error("pgx_tree_content: a level of %u nodes needs %llu workgroups", n_here, blocks);
            return PGX_ERR_INVALID;
        }
        if (h == 0) {
            ProfScope prof(ctx, "tree_leaf_kernel", stream);
            tree_leaf_kernel<<<(uint32_t)blocks, TC_THREADS, 0, stream>>>(d_bits, pgx_bitmap_stride_words(n_genes), n_species, d_leaf,
                                                                          d_order + lo, n_nodes, n_genes, geom, d_counts, d_totals);
        } else {
            ProfScope prof(ctx, "tree_sum_kernel", stream);
            tree_sum_kernel<<<(uint32_t)blocks, TC_THREADS, 0, stream>>>(d_child_off, d_child, n_edges, d_order + lo, n_nodes, geom,
                                                                         d_counts, d_totals);
        }
        PGX_HIP(hipGetLastError());
    }
    return PGX_OK;
}

// What both entries ask of the level offsets (host memory in both): from 0 to n_nodes, never decreasing.
int tree_levels_ok(const uint32_t *level_off, uint32_t n_levels, uint32_t n_nodes) {
    PGX_REQUIRE(level_off, "NULL level_off");
    PGX_REQUIRE(level_off[0] == 0 && level_off[n_levels] == n_nodes, "level_off must run from 0 to n_nodes");
    for (uint32_t h = 0; h < n_levels; ++h) PGX_REQUIRE(level_off[h] <= level_off[h + 1], "level_off must not decrease");
    return PGX_OK;
}

int tree_dev(pgx_ctx *ctx, const u64 *d_bits, uint32_t n_genes, uint32_t n_species, const int32_t *d_leaf,
             const uint32_t *d_child_off, const uint32_t *d_child, uint32_t n_nodes, u64 n_edges, const uint32_t *d_order,
             const uint32_t *level_off, uint32_t n_levels, uint32_t *d_counts, uint32_t *d_totals, void *d_ws, size_t ws_bytes,
             hipStream_t stream) {
    PGX_REQUIRE(ctx, "NULL argument");
    PGX_REQUIRE(tree_sizes_ok(n_nodes, n_genes, n_edges),
                "n_nodes x stride must not pass 2^31 entries, nor the tree 2^31 edges");
    if (n_nodes == 0) return PGX_OK;
    int rc = tree_levels_ok(level_off, n_levels, n_nodes);
    if (rc != PGX_OK) return rc;
    PGX_REQUIRE(d_leaf && d_child_off && d_order && (n_edges == 0 || d_child), "NULL argument");
    PGX_REQUIRE(n_genes == 0 || (d_bits && d_counts), "NULL argument");
    PGX_REQUIRE(d_ws && ws_bytes >= TC_WS_BYTES, "workspace too small (see pgx_tree_content_workspace_bytes)");
    PGX_REQUIRE(((uintptr_t)d_counts & 15u) == 0 && ((uintptr_t)d_ws & 15u) == 0, "d_out_counts and the workspace must be 16-byte aligned");
    return tree_run(ctx, d_bits, n_genes, n_species, d_leaf, d_child_off, d_child, n_nodes, (uint32_t)n_edges, d_order, level_off,
                    n_levels, d_counts, d_totals, stream);
}

// The rules of the host entry (pgx.h, "Gene content of tree nodes"); the message names the first one broken.
int tree_host_check(const int32_t *leaf, const uint32_t *child_off, const uint32_t *child, uint32_t n_nodes, uint32_t n_species,
                    const uint32_t *order, const uint32_t *level_off, uint32_t n_levels) {
    PGX_REQUIRE(child_off[0] == 0, "child_off must start at 0");
    for (uint32_t v = 0; v < n_nodes; ++v) PGX_REQUIRE(child_off[v] <= child_off[v + 1], "child_off must not decrease");
    const uint32_t n_edges = child_off[n_nodes];
    PGX_REQUIRE(n_edges == 0 || child, "NULL child");
    std::vector<uint32_t> level_of(n_nodes, UINT32_MAX);
    std::vector<uint8_t> has_parent(n_nodes, 0);
    for (uint32_t h = 0; h < n_levels; ++h)
        for (uint32_t i = level_off[h]; i < level_off[h + 1]; ++i) {
            const uint32_t v = order[i];
            PGX_REQUIRE(v < n_nodes, "order names a node that does not exist");
            PGX_REQUIRE(level_of[v] == UINT32_MAX, "a node is listed twice in order");
            level_of[v] = h;
        }
    // (n_nodes entries, none twice: every node is listed once)
    for (uint32_t v = 0; v < n_nodes; ++v) {
        PGX_REQUIRE(leaf[v] >= -1, "leaf_species must be a species or -1");
        PGX_REQUIRE(leaf[v] < 0 || (uint32_t)leaf[v] < n_species, "leaf_species must be below n_species");
        const bool mapped = leaf[v] >= 0;
        PGX_REQUIRE(!mapped || level_of[v] == 0, "a mapped node must be listed at height 0");
        PGX_REQUIRE(mapped || level_of[v] > 0 || child_off[v] == child_off[v + 1], "an unmapped node with children is listed at height 0");
        for (uint32_t e = child_off[v]; e < child_off[v + 1]; ++e) {
            const uint32_t x = child[e];
            PGX_REQUIRE(x < n_nodes, "a child is not a node");
            PGX_REQUIRE(!has_parent[x], "a node is a child of two nodes");
            has_parent[x] = 1;
            PGX_REQUIRE(mapped || level_of[x] < level_of[v], "a child of an unmapped node must lie at a lower height");
        }
    }
    return PGX_OK;
}

int tree_host(pgx_ctx *ctx, const int32_t *rows, const int32_t *species, uint64_t n_records, uint32_t n_genes, uint32_t n_species,
              const int32_t *leaf, const uint32_t *child_off, const uint32_t *child, uint32_t n_nodes, const uint32_t *order,
              const uint32_t *level_off, uint32_t n_levels, uint32_t *out_counts, uint32_t *out_totals, uint64_t *out_duplicates) {
    PGX_REQUIRE(ctx, "NULL argument");
    PGX_REQUIRE(n_records == 0 || (rows && species), "NULL record arrays");
    PGX_REQUIRE(child_off, "NULL child_off");
    PGX_REQUIRE(tree_sizes_ok(n_nodes, n_genes, 0), "n_nodes x stride must not pass 2^31 entries");
    if (n_nodes == 0) {
        if (out_duplicates) *out_duplicates = 0;
        return PGX_OK;
    }
    PGX_REQUIRE(leaf && order, "NULL argument");
    PGX_REQUIRE(n_genes == 0 || out_counts, "NULL out_counts");
    int rc = tree_levels_ok(level_off, n_levels, n_nodes);
    if (rc != PGX_OK) return rc;
    rc = tree_host_check(leaf, child_off, child, n_nodes, n_species, order, level_off, n_levels);
    if (rc != PGX_OK) return rc;
    const uint32_t n_edges = child_off[n_nodes];
    PGX_REQUIRE(tree_sizes_ok(n_nodes, n_genes, n_edges), "the tree must not hold more than 2^31 edges");
    PGX_HIP(hipSetDevice(ctx->device_id));
    hipStream_t stream = ctx->stream;
    DevBuf d_bits(ctx, TR_SLOT_BITS), d_cnt(ctx, TR_SLOT_CNT);
    rc = pgx_load_coo_bitmap(ctx, rows, species, n_records, n_genes, n_species, TR_SLOT_ROWS, TR_SLOT_SPECIES, d_bits, d_cnt,
                             out_duplicates);
    if (rc != PGX_OK) return rc;
    const size_t stride = tree_stride(n_genes);
    DevPack in(ctx, TR_SLOT_IN), res(ctx, TR_SLOT_OUT);
    const PackPart i_leaf = in.in(leaf, n_nodes), i_off = in.in(child_off, (size_t)n_nodes + 1), i_child = in.in(child, n_edges),
                   i_order = in.in(order, n_nodes);
    const PackPart o_counts = res.out(out_counts, (size_t)n_nodes * stride), o_totals = res.out(out_totals, n_nodes);
    PGX_HIP(in.alloc());
    PGX_HIP(res.alloc());
    PGX_HIP(in.upload(stream));
    rc = tree_run(ctx, d_bits.as<u64>(), n_genes, n_species, in.dev<int32_t>(i_leaf), in.dev<uint32_t>(i_off),
                  in.dev<uint32_t>(i_child), n_nodes, n_edges, in.dev<uint32_t>(i_order), level_off, n_levels,
                  res.dev<uint32_t>(o_counts), res.dev_if(out_totals, o_totals), stream);
    if (rc != PGX_OK) return rc;
    PGX_HIP(res.download(stream));
    PGX_HIP(hipStreamSynchronize(stream));
    return PGX_OK;
}

}  // namespace

extern "C" {

uint32_t pgx_tree_content_stride(uint32_t n_genes) { return tree_stride(n_genes); }

size_t pgx_tree_content_workspace_bytes(uint32_t n_nodes, uint32_t n_genes, uint64_t n_edges) {
    return tree_sizes_ok(n_nodes, n_genes, n_edges) ? TC_WS_BYTES : 0;
}

int pgx_tree_content(pgx_ctx *ctx, const int32_t *row_of_record, const int32_t *species_of_record, uint64_t n_records,
                     uint32_t n_genes, uint32_t n_species, const int32_t *leaf_species, const uint32_t *child_off,
                     const uint32_t *child, uint32_t n_nodes, const uint32_t *order, const uint32_t *level_off, uint32_t n_levels,
                     uint32_t *out_counts, uint32_t *out_totals, uint64_t *out_duplicates) {
    return guarded(__func__, [&] {
        return tree_host(ctx, row_of_record, species_of_record, n_records, n_genes, n_species, leaf_species, child_off, child,
                         n_nodes, order, level_off, n_levels, out_counts, out_totals, out_duplicates);
    });
}

int pgx_tree_content_dev(pgx_ctx *ctx, const uint64_t *d_bits, uint32_t n_genes, uint32_t n_species,
                         const int32_t *d_leaf_species, const uint32_t *d_child_off, const uint32_t *d_child, uint32_t n_nodes,
                         uint64_t n_edges, const uint32_t *d_order, const uint32_t *level_off, uint32_t n_levels,
                         uint32_t *d_out_counts, uint32_t *d_out_totals, void *d_workspace, size_t workspace_bytes, void *stream) {
    return guarded(__func__, [&] {
        return tree_dev(ctx, (const u64 *)d_bits, n_genes, n_species, d_leaf_species, d_child_off, d_child, n_nodes, n_edges,
                        d_order, level_off, n_levels, d_out_counts, d_out_totals, d_workspace, workspace_bytes, (hipStream_t)stream);
    });
}

}  // extern "C"
