// Shortest-path lengths from many sources to many targets of a directed graph (reference amr.py:289-349 build_resistome calls
// nx.has_path and nx.shortest_path once per (hit, drug): a fresh search of the whole ontology for every pair).
// The graph is successor lists: the successors of node v are succ[succ_off[v] .. succ_off[v + 1]). Self-loops, parallel
// edges and cycles are legal. len[s, t] is the number of NODES on a shortest path from sources[s] to targets[t]: 1 when they
// are the same node, 0 when there is no path.
//
// Every node holds a mask of the targets it reaches, W = ceil(n_targets / 64) words, in two buffers. Round k (k = 1, 2, ...)
// is a pull from the old buffer into the new one,
//     new[v] = old[v] | OR over the successors w of v of old[w]
// so after round k a node's mask holds exactly the targets it reaches over at most k edges: a bit that appears in round k
// stands for a path of k + 1 nodes. Updating one buffer in place would let a bit travel several edges in one round and
// report lengths that are too short. The rounds end with the first one in which no word changed.
//
// Kernels (plain launches on one stream, no atomics):
//   reach_seed_kernel      thread w owns word w of every node: it sets the bits of its 64 targets, one after the other
//   reach_len_seed_kernel  len[s, t] = 1 where sources[s] == targets[t], else 0
//   reach_round_kernel     a group of GR_GROUP lanes owns a node: the lanes take its successors in turn, OR their words
//                          across the group, the group's first lane stores the node's word. A node with more than GR_WIDE
//                          successors is left to the whole workgroup, which does the same with all its lanes. A lane that
//                          stores a word that differs from the old one also stores 1 into `changed`: every writer stores
//                          the same value, the host reads it between rounds.
//   reach_len_kernel       thread (s, w): the bits of sources[s] that are in the new buffer and not in the old one get k + 1
// Ids that are not nodes are skipped by every kernel (the host entry refuses them; the device entry does not look).
#include "pgx_internal.h"

namespace {

typedef unsigned long long u64;

constexpr int GR_THREADS = 256;
constexpr uint32_t GR_GROUP = 16;
constexpr uint32_t GR_NODES_PER_BLOCK = GR_THREADS / GR_GROUP;
constexpr uint32_t GR_WIDE = 512;                          // more successors than this: the workgroup takes the node
constexpr uint32_t GR_MAX_GRID = 8192;
constexpr uint32_t GR_MAX_NODES = 1u << 24, GR_MAX_EDGES = 1u << 31;
constexpr u64 GR_MAX_WORDS = 1ull << 28;                   // n_nodes x W, per buffer
constexpr u64 GR_MAX_CELLS = 1ull << 31;                   // n_sources x n_targets
static_assert(64 % GR_GROUP == 0 && (GR_GROUP & (GR_GROUP - 1)) == 0, "a wave holds whole groups");

__global__ __launch_bounds__(GR_THREADS) void reach_seed_kernel(const uint32_t *__restrict__ targets, uint32_t n_targets,
                                                                uint32_t n_nodes, uint32_t W, u64 *cur) {
    const uint32_t w = blockIdx.x * GR_THREADS + threadIdx.x;
    if (w >= W) return;
    for (uint32_t j = 0; j < 64u; ++j) {
        const uint32_t t = w * 64u + j;
        if (t >= n_targets) break;
        const uint32_t v = targets[t];
        if (v < n_nodes) cur[(size_t)v * W + w] |= 1ull << j;    // (word w of any node is this thread's alone)
    }
}

__global__ __launch_bounds__(GR_THREADS) void reach_len_seed_kernel(const uint32_t *__restrict__ sources, uint32_t n_sources,
                                                                    const uint32_t *__restrict__ targets, uint32_t n_targets,
                                                                    uint32_t n_nodes, uint32_t *__restrict__ out) {
    const u64 cells = (u64)n_sources * n_targets;
    for (u64 i = (u64)blockIdx.x * GR_THREADS + threadIdx.x; i < cells; i += (u64)gridDim.x * GR_THREADS) {
        const uint32_t v = sources[i / n_targets];
        out[i] = v < n_nodes && v == targets[i % n_targets] ? 1u : 0u;
    }
}

__device__ __forceinline__ void node_span(const uint32_t *__restrict__ succ_off, uint32_t v, uint32_t n_edges, uint32_t &begin,
                                          uint32_t &end) {
    begin = succ_off[v];
    end = succ_off[v + 1];
    if (begin > n_edges) begin = n_edges;
    if (end > n_edges) end = n_edges;
    if (end < begin) end = begin;
}

__global__ __launch_bounds__(GR_THREADS) void reach_round_kernel(const uint32_t *__restrict__ succ_off,
                                                                 const uint32_t *__restrict__ succ, uint32_t n_nodes,
                                                                 uint32_t n_edges, uint32_t W, const u64 *__restrict__ old,
                                                                 u64 *__restrict__ cur, uint32_t *changed) {
    __shared__ u64 s_part[GR_THREADS / 64];
    const uint32_t tid = threadIdx.x, sub = tid & (GR_GROUP - 1u), grp = tid / GR_GROUP;
    const uint32_t n_rounds = (n_nodes + GR_NODES_PER_BLOCK - 1u) / GR_NODES_PER_BLOCK;
    // every lane takes the same rounds and the same words, so the shuffles and barriers are reached by whole workgroups
    for (uint32_t round = blockIdx.x; round < n_rounds; round += gridDim.x) {
        const uint32_t v = round * GR_NODES_PER_BLOCK + grp;
        const bool live = v < n_nodes;
        uint32_t begin = 0, end = 0;
        if (live) node_span(succ_off, v, n_edges, begin, end);
        const bool mine = live && end - begin <= GR_WIDE;
        for (uint32_t w = 0; w < W; ++w) {
            u64 acc = 0;
            if (mine)
                for (uint32_t e = begin + sub; e < end; e += GR_GROUP) {
                    const uint32_t x = succ[e];
                    if (x < n_nodes) acc |= old[(size_t)x * W + w];
                }
            for (int d = GR_GROUP / 2; d >= 1; d >>= 1) acc |= __shfl_xor(acc, d, 64);
            if (mine && sub == 0u) {
                const u64 o = old[(size_t)v * W + w], r = o | acc;
                cur[(size_t)v * W + w] = r;
                if (r != o) *changed = 1u;
            }
        }
        for (uint32_t g = 0; g < GR_NODES_PER_BLOCK; ++g) {          // the wide nodes of this round, one after the other
            const uint32_t u = round * GR_NODES_PER_BLOCK + g;
            if (u >= n_nodes) break;
            uint32_t b, e_end;
            node_span(succ_off, u, n_edges, b, e_end);
            if (e_end - b <= GR_WIDE) continue;
            for (uint32_t w = 0; w < W; ++w) {
                u64 acc = 0;
                for (uint32_t e = b + tid; e < e_end; e += GR_THREADS) {
                    const uint32_t x = succ[e];
                    if (x < n_nodes) acc |= old[(size_t)x * W + w];
                }
                for (int d = 32; d >= 1; d >>= 1) acc |= __shfl_xor(acc, d, 64);
                if ((tid & 63u) == 0u) s_part[tid >> 6] = acc;
                __syncthreads();
                if (tid == 0u) {
                    u64 r = old[(size_t)u * W + w];
                    const u64 o = r;
                    for (int p = 0; p < GR_THREADS / 64; ++p) r |= s_part[p];
                    cur[(size_t)u * W + w] = r;
                    if (r != o) *changed = 1u;
                }
                __syncthreads();
            }
        }
    }
}

__global__ __launch_bounds__(GR_THREADS) void reach_len_kernel(const uint32_t *__restrict__ sources, uint32_t n_sources,
                                                               uint32_t n_targets, uint32_t n_nodes, uint32_t W,
                                                               const u64 *__restrict__ old, const u64 *__restrict__ cur,
                                                               uint32_t level, uint32_t *__restrict__ out) {
    const u64 items = (u64)n_sources * W;
    for (u64 i = (u64)blockIdx.x * GR_THREADS + threadIdx.x; i < items; i += (u64)gridDim.x * GR_THREADS) {
        const uint32_t s = (uint32_t)(i / W), w = (uint32_t)(i % W);
        const uint32_t v = sources[s];
        if (v >= n_nodes) continue;
        u64 fresh = cur[(size_t)v * W + w] & ~old[(size_t)v * W + w];
        while (fresh) {
            const uint32_t t = w * 64u + (uint32_t)__builtin_ctzll(fresh);
            fresh &= fresh - 1ull;
            if (t < n_targets) out[(size_t)s * n_targets + t] = level;
        }
    }
}

// ---- launches ------------------------------------------------------------------------------------------------------------
struct ReachWs {
    size_t a, b, changed, bytes;
    uint32_t W;
};

bool reach_sizes_ok(uint32_t n_nodes, uint32_t n_targets, uint32_t n_sources) {
    const u64 W = ((u64)n_targets + 63u) / 64u;
    return n_nodes < GR_MAX_NODES && (u64)n_nodes * W < GR_MAX_WORDS && (u64)n_sources * n_targets < GR_MAX_CELLS;
}

ReachWs reach_layout(uint32_t n_nodes, uint32_t n_targets) {
    ReachWs r;
    WsLayout lay;
    r.W = (n_targets + 63u) / 64u;
    r.a = lay.take((size_t)n_nodes * r.W * 8);
    r.b = lay.take((size_t)n_nodes * r.W * 8);
    r.changed = lay.take(4);
    r.bytes = lay.off;
    return r;
}

uint32_t grid_for(u64 items, uint32_t per_block) {
    const u64 blocks = (items + per_block - 1) / per_block;
    return blocks < 1 ? 1u : blocks < GR_MAX_GRID ? (uint32_t)blocks : GR_MAX_GRID;
}

int reach_require(pgx_ctx *ctx, uint32_t n_nodes, u64 n_edges, uint32_t n_targets, uint32_t n_sources) {
    PGX_REQUIRE(ctx, "NULL argument");
    PGX_REQUIRE(n_nodes < GR_MAX_NODES, "n_nodes must be below 2^24");
    PGX_REQUIRE(n_edges < GR_MAX_EDGES, "the graph must hold fewer than 2^31 edges");
    PGX_REQUIRE(reach_sizes_ok(n_nodes, n_targets, n_sources),
                "n_nodes x ceil(n_targets / 64) must be below 2^28 and n_sources x n_targets below 2^31");
    return PGX_OK;
}

// Everything on the device; `stream` is synchronised once per round (the host reads `changed`). *rounds: the rounds run.
int reach_run(pgx_ctx *ctx, const uint32_t *d_succ_off, const uint32_t *d_succ, uint32_t n_nodes, uint32_t n_edges,
              const uint32_t *d_targets, uint32_t n_targets, const uint32_t *d_sources, uint32_t n_sources, uint32_t *d_out,
              char *ws, hipStream_t stream, uint32_t *rounds) {
    const ReachWs lay = reach_layout(n_nodes, n_targets);
    const uint32_t W = lay.W;
    u64 *old = (u64 *)(ws + lay.a), *cur = (u64 *)(ws + lay.b);
    uint32_t *d_changed = (uint32_t *)(ws + lay.changed);
    const u64 cells = (u64)n_sources * n_targets;
    PGX_HIP(hipMemsetAsync(old, 0, (size_t)n_nodes * W * 8, stream));
    {
        ProfScope prof(ctx, "reach_seed_kernel", stream);
        reach_seed_kernel<<<grid_for(W, GR_THREADS), GR_THREADS, 0, stream>>>(d_targets, n_targets, n_nodes, W, old);
        reach_len_seed_kernel<<<grid_for(cells, GR_THREADS), GR_THREADS, 0, stream>>>(d_sources, n_sources, d_targets, n_targets,
                                                                                     n_nodes, d_out);
    }
    PGX_HIP(hipGetLastError());
    *rounds = 0;
    if (n_nodes == 0) return PGX_OK;
    // a round without a new bit ends the loop; bits are never cleared and a shortest path holds at most n_nodes nodes, so
    // that round comes after n_nodes rounds at the latest
    for (;;) {
        uint32_t changed = 0;
        PGX_HIP(hipMemsetAsync(d_changed, 0, 4, stream));
        {
            ProfScope prof(ctx, "reach_round_kernel", stream);
            reach_round_kernel<<<grid_for(n_nodes, GR_NODES_PER_BLOCK), GR_THREADS, 0, stream>>>(d_succ_off, d_succ, n_nodes,
                                                                                                n_edges, W, old, cur, d_changed);
        }
        {
            ProfScope prof(ctx, "reach_len_kernel", stream);
            reach_len_kernel<<<grid_for((u64)n_sources * W, GR_THREADS), GR_THREADS, 0, stream>>>(
                d_sources, n_sources, n_targets, n_nodes, W, old, cur, *rounds + 2u, d_out);
        }
        PGX_HIP(hipGetLastError());
        PGX_HIP(hipMemcpyAsync(&changed, d_changed, 4, hipMemcpyDeviceToHost, stream));
        PGX_HIP(hipStreamSynchronize(stream));
        ++*rounds;
        std::swap(old, cur);
        if (!changed) break;
        if (*rounds > n_nodes) {
            pgx_set_error("pgx_graph_reach: the masks still change after n_nodes rounds");
            return PGX_ERR_INTERNAL;
        }
    }
    return PGX_OK;
}

int reach_dev(pgx_ctx *ctx, const uint32_t *d_succ_off, const uint32_t *d_succ, uint32_t n_nodes, uint32_t n_edges,
              const uint32_t *d_targets, uint32_t n_targets, const uint32_t *d_sources, uint32_t n_sources, uint32_t *d_out,
              uint32_t *d_rounds, void *d_ws, size_t ws_bytes, hipStream_t stream) {
    int rc = reach_require(ctx, n_nodes, n_edges, n_targets, n_sources);
    if (rc != PGX_OK) return rc;
    if (n_sources == 0 || n_targets == 0) return PGX_OK;
    PGX_REQUIRE(d_succ_off && d_targets && d_sources && d_out && (n_edges == 0 || d_succ), "NULL argument");
    PGX_REQUIRE(d_ws && ws_bytes >= reach_layout(n_nodes, n_targets).bytes,
                "workspace too small (see pgx_graph_reach_workspace_bytes)");
    PGX_REQUIRE(((uintptr_t)d_ws & 15u) == 0, "workspace must be 16-byte aligned");
    uint32_t rounds = 0;
    rc = reach_run(ctx, d_succ_off, d_succ, n_nodes, n_edges, d_targets, n_targets, d_sources, n_sources, d_out, (char *)d_ws,
                   stream, &rounds);
    if (rc != PGX_OK) return rc;
    if (d_rounds) PGX_HIP(hipMemcpyAsync(d_rounds, &rounds, 4, hipMemcpyHostToDevice, stream));
    PGX_HIP(hipStreamSynchronize(stream));
    return PGX_OK;
}

int reach_host(pgx_ctx *ctx, const uint32_t *succ_off, const uint32_t *succ, uint32_t n_nodes, const uint32_t *targets,
               uint32_t n_targets, const uint32_t *sources, uint32_t n_sources, uint32_t *out_len, uint32_t *out_rounds) {
    PGX_REQUIRE(ctx, "NULL argument");
    PGX_REQUIRE(n_nodes < GR_MAX_NODES, "n_nodes must be below 2^24");
    PGX_REQUIRE(succ_off, "NULL succ_off");
    for (uint32_t v = 0; v < n_nodes; ++v) PGX_REQUIRE(succ_off[v] <= succ_off[v + 1], "offsets must not decrease");
    PGX_REQUIRE(succ_off[0] == 0, "offsets must start at 0");
    const uint32_t n_edges = succ_off[n_nodes];
    int rc = reach_require(ctx, n_nodes, n_edges, n_targets, n_sources);
    if (rc != PGX_OK) return rc;
    PGX_REQUIRE(n_edges == 0 || succ, "NULL succ");
    PGX_REQUIRE((n_targets == 0 || targets) && (n_sources == 0 || sources), "NULL targets or sources");
    for (uint32_t e = 0; e < n_edges; ++e) PGX_REQUIRE(succ[e] < n_nodes, "a successor is not a node");
    for (uint32_t t = 0; t < n_targets; ++t) PGX_REQUIRE(targets[t] < n_nodes, "a target is not a node");
    for (uint32_t s = 0; s < n_sources; ++s) PGX_REQUIRE(sources[s] < n_nodes, "a source is not a node");
    if (n_sources == 0 || n_targets == 0) return PGX_OK;
    PGX_REQUIRE(out_len, "NULL out_len");
    PGX_HIP(hipSetDevice(ctx->device_id));
    DevPack in(ctx, GR_SLOT_IN), res(ctx, GR_SLOT_OUT);
    DevBuf d_ws(ctx, GR_SLOT_WS);
    const PackPart p_off = in.in(succ_off, (size_t)n_nodes + 1), p_succ = in.in(succ, n_edges),
                   p_tgt = in.in(targets, n_targets), p_src = in.in(sources, n_sources);
    const PackPart r_len = res.out(out_len, (size_t)n_sources * n_targets);
    PGX_HIP(in.alloc());
    PGX_HIP(res.alloc());
    PGX_HIP(d_ws.alloc(reach_layout(n_nodes, n_targets).bytes));
    PGX_HIP(in.upload(ctx->stream));
    uint32_t rounds = 0;
    rc = reach_run(ctx, in.dev<uint32_t>(p_off), in.dev<uint32_t>(p_succ), n_nodes, n_edges, in.dev<uint32_t>(p_tgt), n_targets,
                   in.dev<uint32_t>(p_src), n_sources, res.dev<uint32_t>(r_len), d_ws.as<char>(), ctx->stream, &rounds);
    if (rc != PGX_OK) return rc;
    PGX_HIP(res.download(ctx->stream));
    PGX_HIP(hipStreamSynchronize(ctx->stream));
    if (out_rounds) *out_rounds = rounds;
    return PGX_OK;
}

}  // namespace

extern "C" {

size_t pgx_graph_reach_workspace_bytes(uint32_t n_nodes, uint32_t n_targets, uint32_t n_sources) {
    if (!reach_sizes_ok(n_nodes, n_targets, n_sources)) return 0;
    return reach_layout(n_nodes, n_targets).bytes;
}

int pgx_graph_reach(pgx_ctx *ctx, const uint32_t *succ_off, const uint32_t *succ, uint32_t n_nodes, const uint32_t *targets,
                    uint32_t n_targets, const uint32_t *sources, uint32_t n_sources, uint32_t *out_len, uint32_t *out_rounds) {
    return guarded(__func__, [&] {
        return reach_host(ctx, succ_off, succ, n_nodes, targets, n_targets, sources, n_sources, out_len, out_rounds);
    });
}

int pgx_graph_reach_dev(pgx_ctx *ctx, const uint32_t *d_succ_off, const uint32_t *d_succ, uint32_t n_nodes, uint64_t n_edges,
                        const uint32_t *d_targets, uint32_t n_targets, const uint32_t *d_sources, uint32_t n_sources,
                        uint32_t *d_out_len, uint32_t *d_out_rounds, void *d_workspace, size_t workspace_bytes, void *stream) {
    return guarded(__func__, [&]() -> int {
        if (n_edges >= GR_MAX_EDGES) {
            pgx_set_error("pgx_graph_reach_dev: the graph must hold fewer than 2^31 edges");
            return PGX_ERR_INVALID;
        }
        return reach_dev(ctx, d_succ_off, d_succ, n_nodes, (uint32_t)n_edges, d_targets, n_targets, d_sources, n_sources,
                         d_out_len, d_out_rounds, d_workspace, workspace_bytes, (hipStream_t)stream);
    });
}

}  // extern "C"
