// Exact multi-pattern matching of variable-length patterns (the primitive behind pangenomix_amd.mlst; reference
// pangenome_analysis.py:402-453 run_mlst shells out to an external typing tool): for every pattern, WHERE it first occurs in
// the text and HOW OFTEN. Pattern k is the bytes [offsets[k], offsets[k + 1]) of a blob, L_k of them;
//   first[k] = the smallest i with text[i .. i + L_k) == pattern k, 0xFFFFFFFF for none
//   count[k] = the number of such i (overlapping occurrences each count)
// Bytes are bytes: no case folding, no alphabet; contigs and strands are the caller's business.
//
// Only the first `seed` bytes of a pattern are hashed (scan.hip's two polynomial hashes, mixed to 64 bits), and the hash only
// decides WHERE to look: an occurrence is counted after all L_k bytes have been compared, so the result is exact whatever
// the hash does -- PGX_PATTERN_NARROW_HASH keeps 3 bits of it and must give the same output. The layout is scan.hip's:
//   bits 0-17 of the hash    the seed's bit in a 2^18-bit filter (32 KiB, a copy of it sits in LDS beside the tile)
//   bits 18-...              the first slot probed in an open-addressed table of 64-bit entries, linear probing
//   bits 24-63               the entry's 40-bit tag; its low 24 bits are the pattern's index (n_patterns < 2^24, so an entry is
//                            never the all-ones word that marks an empty slot)
// The table has at least twice as many slots as patterns, so a probe sequence always reaches an empty slot; nothing is ever
// removed, so every pattern whose seed hashes like a position's lies between that position's first slot and the next empty
// one. Patterns that share a seed are a run of equal-tag entries: the normal case for the alleles of one locus.
//
// Kernels (plain launches on one stream):
//   pattern_build_kernel  one lane per pattern: hash of its seed, atomicOr of the filter bit, insertion with atomicCAS on the
//                         first empty slot. A pattern shorter than the seed (the host entries refuse it) is not inserted.
//   pattern_scan_kernel   a workgroup copies the filter to LDS, then takes tiles of PT_TILE text positions. The tile and a halo
//                         of seed - 1 bytes are staged in LDS (nothing at or beyond text_bytes is read); lane l hashes the seeds
//                         at positions l, l + 256, ..., tests the filter and walks the table ALONE up to the first tag match
//                         or an empty slot. Then the wave verifies together: the lanes that met a tag are balloted and taken
//                         one at a time, position and hash are broadcast, all 64 lanes walk that chain again, and for every
//                         equal-tag entry whose pattern fits before text_bytes they compare pattern and text 16 bytes per
//                         lane and 1 KiB per step (string_hash.h load_chunk: aligned 16-byte loads inside the buffers, bytes
//                         at their edges), one ballot per step ending a pattern at its first difference. Lane 0 then does
//                         atomicMin(first[k]) and atomicAdd(count[k]): a minimum and an integer sum over a set, so the same
//                         input gives the same bytes on every call.
//                         Every lane of a wave reaches every ballot: a lane with no position left takes part with "no hit",
//                         and nothing between the ballot and the end of the verification is a workgroup barrier.
//                         The text beyond the seed is read from global memory: a pattern may be longer than a tile.
#include "pgx_internal.h"
#include "string_hash.h"

namespace {

using string_hash::Chunk;
using string_hash::load_chunk;
using string_hash::string_span;
typedef unsigned long long u64;

constexpr int PT_THREADS = 256;
constexpr uint32_t PT_TILE = 4096;                       // text positions per tile (pgx_pattern_scan_tile)
constexpr uint32_t PT_MAX_SEED = 64;
constexpr uint32_t PT_TILE_BYTES = PT_TILE + PT_MAX_SEED;           // tile + halo (seed - 1 <= 63), a multiple of 16
constexpr uint32_t PT_FILTER_LOG2 = 18;
constexpr uint32_t PT_FILTER_WORDS = (1u << PT_FILTER_LOG2) / 32;   // 8192 words = 32 KiB
constexpr uint32_t PT_MAX_GRID = 2048;
constexpr uint32_t PT_CHUNK = 16;                        // bytes per lane and step of a comparison
constexpr u64 PT_EMPTY = ~0ull;
static_assert(PT_TILE_BYTES % 16 == 0 && PT_TILE_BYTES + PT_FILTER_WORDS * 4 <= 64 * 1024, "static LDS stays under 64 KiB");

struct PatternGeom {
    uint32_t slots;                   // a power of two, >= 2 * n_patterns
    size_t off_table, off_filter, bytes;
};

bool sizes_ok(uint64_t pattern_bytes, uint32_t n_patterns) { return pattern_bytes < (1ull << 32) && n_patterns < (1u << 24); }

PatternGeom make_geom(uint32_t n_patterns) {
    PatternGeom g;
    g.slots = 64;
    while (g.slots < 2 * n_patterns) g.slots <<= 1;       // (n_patterns < 2^24: at most 2^25)
    g.off_table = 0;
    g.off_filter = (size_t)g.slots * 8;                   // (a multiple of 256)
    g.bytes = g.off_filter + (size_t)PT_FILTER_WORDS * 4;
    return g;
}

// scan.hip's hash and slot helpers, restated (its kernels stay as they are)
struct Hash2 {
    uint32_t a = 0x9E3779B9u, b = 0x85EBCA6Bu;
    __device__ __forceinline__ void add(uint32_t byte) {
        a = a * 0x01000193u + byte + 1u;
        b = (b ^ byte) * 0x2C1B3C6Du + 0x297A2D39u;
    }
    __device__ __forceinline__ u64 value(uint32_t flags) const {
        u64 h = ((u64)b << 32) | a;
        h ^= h >> 33; h *= 0xFF51AFD7ED558CCDull;
        h ^= h >> 33; h *= 0xC4CEB9FE1A85EC53ull;
        h ^= h >> 33;
        return (flags & PGX_PATTERN_NARROW_HASH) ? (h & 7ull) : h;
    }
};

__device__ __forceinline__ uint32_t filter_bit(u64 h) { return (uint32_t)h & ((1u << PT_FILTER_LOG2) - 1u); }
__device__ __forceinline__ uint32_t first_slot(u64 h, uint32_t mask) { return (uint32_t)(h >> PT_FILTER_LOG2) & mask; }
__device__ __forceinline__ u64 tag_of(u64 h) { return h >> 24; }

__global__ __launch_bounds__(PT_THREADS) void pattern_build_kernel(const uint8_t *__restrict__ patterns,
                                                                   const u64 *__restrict__ offsets, uint32_t n_patterns,
                                                                   uint32_t seed, uint32_t flags, u64 *table, uint32_t mask,
                                                                   uint32_t *__restrict__ filter) {
    const uint32_t k = blockIdx.x * PT_THREADS + threadIdx.x;
    if (k >= n_patterns) return;
    u64 begin, len;
    string_span(offsets, k, offsets[n_patterns], begin, len);
    if (len < seed) return;                                  // (no seed to hash: the pattern matches nowhere)
    Hash2 hs;
    for (uint32_t j = 0; j < seed; ++j) hs.add(patterns[begin + j]);
    const u64 h = hs.value(flags);
    const uint32_t bit = filter_bit(h);
    atomicOr(&filter[bit >> 5], 1u << (bit & 31u));
    const u64 entry = (tag_of(h) << 24) | k;
    uint32_t s = first_slot(h, mask);
    // `mask + 1` >= 2 * n_patterns slots, of which fewer than n_patterns are taken: an empty one is always met
    for (;;) {
        if (__atomic_load_n(&table[s], __ATOMIC_RELAXED) == PT_EMPTY && atomicCAS(&table[s], PT_EMPTY, entry) == PT_EMPTY)
            break;
        s = (s + 1u) & mask;
    }
}

__global__ __launch_bounds__(PT_THREADS) void pattern_scan_kernel(const uint8_t *__restrict__ text, uint32_t text_bytes,
                                                                  const uint8_t *__restrict__ patterns,
                                                                  const u64 *__restrict__ offsets, uint32_t n_patterns,
                                                                  uint32_t seed, uint32_t flags, const u64 *__restrict__ table,
                                                                  uint32_t mask, const uint32_t *__restrict__ filter,
                                                                  uint32_t n_tiles, uint32_t *__restrict__ first,
                                                                  uint32_t *__restrict__ count) {
    __shared__ uint4 s_tile4[PT_TILE_BYTES / 16];
    __shared__ uint4 s_filter4[PT_FILTER_WORDS / 4];
    uint8_t *s_tile = reinterpret_cast<uint8_t *>(s_tile4);
    const uint32_t *s_filter = reinterpret_cast<const uint32_t *>(s_filter4);
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    for (uint32_t i = tid; i < PT_FILTER_WORDS / 4; i += PT_THREADS)
        s_filter4[i] = reinterpret_cast<const uint4 *>(filter)[i];              // (the workspace is 16-byte aligned)
    const u64 total = offsets[n_patterns];
    const uint32_t n_pos = text_bytes - seed + 1u;                               // the caller has text_bytes >= seed
    const bool aligned = (reinterpret_cast<uintptr_t>(text) & 15u) == 0;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t t0 = tile * PT_TILE;                                      // < n_pos <= 2^32 - 1
        const uint32_t left = text_bytes - t0;
        const uint32_t have = left < PT_TILE + seed - 1u ? left : PT_TILE + seed - 1u;   // bytes staged, <= PT_TILE_BYTES
        __syncthreads();                                                         // the tile before this one has been read
        const uint32_t whole = aligned ? have / 16u : 0u;                        // t0 is a multiple of 16
        for (uint32_t i = tid; i < whole; i += PT_THREADS)
            s_tile4[i] = reinterpret_cast<const uint4 *>(text + t0)[i];
        for (uint32_t i = whole * 16u + tid; i < have; i += PT_THREADS) s_tile[i] = text[(size_t)t0 + i];
        __syncthreads();
        const uint32_t pos_here = n_pos - t0 < PT_TILE ? n_pos - t0 : PT_TILE;
        // r and pos_here are the same on every lane of the workgroup: whole waves take every round, a lane without a
        // position votes "no hit"
        for (uint32_t r = 0; r * PT_THREADS < pos_here; ++r) {
            const uint32_t p = r * PT_THREADS + tid;                             // p + seed <= have where p < pos_here
            bool hit = false;
            u64 h = 0;
            if (p < pos_here) {
                Hash2 hs;
                for (uint32_t j = 0; j < seed; ++j) hs.add(s_tile[p + j]);
                h = hs.value(flags);
                const uint32_t bit = filter_bit(h);
                if ((s_filter[bit >> 5] >> (bit & 31u)) & 1u) {
                    const u64 tag = tag_of(h);
                    for (uint32_t s = first_slot(h, mask);; s = (s + 1u) & mask) {
                        const u64 e = table[s];
                        if (e == PT_EMPTY) break;
                        if ((e >> 24) == tag) { hit = true; break; }
                    }
                }
            }
            u64 votes = __ballot(hit);
            while (votes) {                                                      // (the same on every lane)
                const int src = __ffsll((long long)votes) - 1;
                votes &= votes - 1ull;
                const uint32_t gp = (uint32_t)__shfl((int)(t0 + p), src, 64);    // the position in the text
                const u64 hh = ((u64)(uint32_t)__shfl((int)(uint32_t)(h >> 32), src, 64) << 32) |
                               (uint32_t)__shfl((int)(uint32_t)h, src, 64);
                const u64 tag = tag_of(hh);
                for (uint32_t s = first_slot(hh, mask);; s = (s + 1u) & mask) {
                    const u64 e = table[s];
                    if (e == PT_EMPTY) break;
                    if ((e >> 24) != tag) continue;
                    const uint32_t k = (uint32_t)e & 0xFFFFFFu;
                    u64 begin, len;
                    string_span(offsets, k, total, begin, len);
                    if (len < seed || (u64)gp + len > text_bytes) continue;       // it would run past the text
                    const u64 n_chunks = (len + PT_CHUNK - 1) / PT_CHUNK;
                    bool equal = true;
                    for (u64 base = 0; base < n_chunks; base += 64) {
                        const u64 c = base + lane;
                        bool differs = false;
                        if (c < n_chunks) {
                            const u64 rest = len - c * PT_CHUNK;
                            const uint32_t n = rest < PT_CHUNK ? (uint32_t)rest : PT_CHUNK;
                            const Chunk a = load_chunk(patterns, total, begin + c * PT_CHUNK, n);
                            const Chunk b = load_chunk(text, text_bytes, (u64)gp + c * PT_CHUNK, n);
                            differs = (a.lo != b.lo) | (a.hi != b.hi);
                        }
                        if (__ballot(differs)) { equal = false; break; }
                    }
                    if (equal && lane == 0u) {
                        atomicMin(&first[k], gp);
                        atomicAdd(&count[k], 1u);
                    }
                }
            }
        }
    }
}

int pattern_sizes(pgx_ctx *ctx, uint32_t n_patterns, uint32_t seed, uint32_t flags) {
    PGX_REQUIRE(ctx, "NULL argument");
    PGX_REQUIRE(seed >= 1 && seed <= PT_MAX_SEED, "seed must be 1..64");
    PGX_REQUIRE(n_patterns < (1u << 24), "n_patterns must be below 2^24");
    PGX_REQUIRE((flags & ~PGX_PATTERN_NARROW_HASH) == 0, "unknown flags");
    return PGX_OK;
}

// table and filter of the set, enqueued on `stream`
int pattern_build(pgx_ctx *ctx, const uint8_t *d_patterns, const u64 *d_offsets, uint32_t n_patterns, uint32_t seed,
                  uint32_t flags, void *d_ws, hipStream_t stream) {
    const PatternGeom g = make_geom(n_patterns);
    u64 *table = (u64 *)((char *)d_ws + g.off_table);
    uint32_t *filter = (uint32_t *)((char *)d_ws + g.off_filter);
    PGX_HIP(hipMemsetAsync(table, 0xFF, (size_t)g.slots * 8, stream));
    PGX_HIP(hipMemsetAsync(filter, 0, (size_t)PT_FILTER_WORDS * 4, stream));
    {
        ProfScope prof(ctx, "pattern_build_kernel", stream);
        pattern_build_kernel<<<ceil_div_u32(n_patterns, PT_THREADS), PT_THREADS, 0, stream>>>(d_patterns, d_offsets, n_patterns,
                                                                                             seed, flags, table, g.slots - 1u,
                                                                                             filter);
    }
    PGX_HIP(hipGetLastError());
    return PGX_OK;
}

// first = 0xFFFFFFFF, count = 0, then the scan where the text holds a seed; enqueued on `stream`. n_patterns >= 1.
int pattern_scan(pgx_ctx *ctx, const uint8_t *d_text, uint64_t text_bytes, const uint8_t *d_patterns, const u64 *d_offsets,
                 uint32_t n_patterns, uint32_t seed, uint32_t flags, const void *d_ws, uint32_t *d_first, uint32_t *d_count,
                 hipStream_t stream) {
    PGX_HIP(hipMemsetAsync(d_first, 0xFF, (size_t)n_patterns * 4, stream));
    PGX_HIP(hipMemsetAsync(d_count, 0, (size_t)n_patterns * 4, stream));
    if (text_bytes < seed) return PGX_OK;
    const PatternGeom g = make_geom(n_patterns);
    const u64 *table = (const u64 *)((const char *)d_ws + g.off_table);
    const uint32_t *filter = (const uint32_t *)((const char *)d_ws + g.off_filter);
    const uint64_t n_pos = text_bytes - seed + 1u;
    const uint32_t n_tiles = (uint32_t)((n_pos + PT_TILE - 1) / PT_TILE);
    {
        ProfScope prof(ctx, "pattern_scan_kernel", stream);
        pattern_scan_kernel<<<std::min(n_tiles, PT_MAX_GRID), PT_THREADS, 0, stream>>>(d_text, (uint32_t)text_bytes, d_patterns,
                                                                                      d_offsets, n_patterns, seed, flags, table,
                                                                                      g.slots - 1u, filter, n_tiles, d_first,
                                                                                      d_count);
    }
    PGX_HIP(hipGetLastError());
    return PGX_OK;
}

// Everything on the device; `stream` is synchronised once, at the end.
int pattern_scan_dev(pgx_ctx *ctx, const uint8_t *d_text, uint64_t text_bytes, const uint8_t *d_patterns, const u64 *d_offsets,
                     uint32_t n_patterns, uint32_t seed, uint32_t flags, uint32_t *d_first, uint32_t *d_count, void *d_ws,
                     size_t ws_bytes, hipStream_t stream) {
    int rc = pattern_sizes(ctx, n_patterns, seed, flags);
    if (rc != PGX_OK) return rc;
    PGX_REQUIRE(text_bytes < (1ull << 32), "text_bytes must be below 2^32");
    if (n_patterns == 0) return PGX_OK;
    PGX_REQUIRE(d_patterns && d_offsets && d_first && d_count, "NULL patterns, offsets, first or count");
    PGX_REQUIRE(text_bytes == 0 || d_text, "NULL text");
    PGX_REQUIRE(((uintptr_t)d_offsets & 7u) == 0, "offsets must be 8-byte aligned");
    PGX_REQUIRE(((uintptr_t)d_first & 3u) == 0 && ((uintptr_t)d_count & 3u) == 0, "first and count must be 4-byte aligned");
    PGX_REQUIRE(d_ws && ws_bytes >= make_geom(n_patterns).bytes, "workspace too small (see pgx_pattern_workspace_bytes)");
    PGX_REQUIRE(((uintptr_t)d_ws & 15u) == 0, "workspace must be 16-byte aligned");
    if (text_bytes >= seed) {
        rc = pattern_build(ctx, d_patterns, d_offsets, n_patterns, seed, flags, d_ws, stream);
        if (rc != PGX_OK) return rc;
    }
    rc = pattern_scan(ctx, d_text, text_bytes, d_patterns, d_offsets, n_patterns, seed, flags, d_ws, d_first, d_count, stream);
    if (rc != PGX_OK) return rc;
    PGX_HIP(hipStreamSynchronize(stream));
    return PGX_OK;
}

int pattern_load_host(pgx_ctx *ctx, const uint8_t *patterns, const uint64_t *offsets, uint32_t n_patterns, uint32_t seed,
                      uint32_t flags) {
    int rc = pattern_sizes(ctx, n_patterns, seed, flags);
    if (rc != PGX_OK) return rc;
    PGX_REQUIRE(offsets, "NULL pattern_offsets");
    for (uint32_t k = 0; k < n_patterns; ++k) {
        PGX_REQUIRE(offsets[k] <= offsets[k + 1], "offsets must not decrease");
        PGX_REQUIRE(offsets[k + 1] - offsets[k] >= seed, "a pattern is shorter than the seed");
    }
    PGX_REQUIRE(offsets[n_patterns] < (1ull << 32), "a blob must hold fewer than 2^32 bytes");
    PGX_REQUIRE(offsets[n_patterns] == 0 || patterns, "NULL patterns");
    PGX_HIP(hipSetDevice(ctx->device_id));
    ctx->pattern_loaded = false;
    const size_t bytes = (size_t)offsets[n_patterns];
    DevBuf d_blob(ctx, PT_SLOT_PATTERNS), d_off(ctx, PT_SLOT_OFFSETS), d_ws(ctx, PT_SLOT_WS);
    PGX_HIP(d_blob.alloc(bytes));
    PGX_HIP(d_off.alloc(((size_t)n_patterns + 1) * 8));
    PGX_HIP(d_ws.alloc(make_geom(n_patterns).bytes));
    if (bytes) {
        rc = pgx_staged_h2d(ctx, d_blob.p, patterns, bytes, ctx->stream);
        if (rc != PGX_OK) return rc;
    }
    PGX_HIP(hipMemcpyAsync(d_off.p, offsets, ((size_t)n_patterns + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    if (n_patterns) {
        rc = pattern_build(ctx, d_blob.as<uint8_t>(), d_off.as<u64>(), n_patterns, seed, flags, d_ws.p, ctx->stream);
        if (rc != PGX_OK) return rc;
    }
    PGX_HIP(hipStreamSynchronize(ctx->stream));
    ctx->pattern_loaded = true;
    ctx->pattern_count = n_patterns;
    ctx->pattern_seed = seed;
    ctx->pattern_flags = flags;
    ctx->pattern_d_blob = d_blob.p;
    ctx->pattern_d_offsets = d_off.p;
    ctx->pattern_d_ws = d_ws.p;
    return PGX_OK;
}

int pattern_query_host(pgx_ctx *ctx, const uint8_t *text, uint64_t text_bytes, uint32_t *out_first, uint32_t *out_count) {
    PGX_REQUIRE(ctx, "NULL argument");
    PGX_REQUIRE(ctx->pattern_loaded, "no set of patterns is loaded (pgx_pattern_load)");
    PGX_REQUIRE(text_bytes < (1ull << 32), "text_bytes must be below 2^32");
    const uint32_t n = ctx->pattern_count, seed = ctx->pattern_seed;
    if (n == 0) return PGX_OK;
    PGX_REQUIRE(out_first && out_count, "NULL out_first or out_count");
    PGX_REQUIRE(text_bytes == 0 || text, "NULL text");
    if (text_bytes < seed) {                                                     // no seed: nothing to upload
        memset(out_first, 0xFF, (size_t)n * 4);
        memset(out_count, 0, (size_t)n * 4);
        return PGX_OK;
    }
    PGX_HIP(hipSetDevice(ctx->device_id));
    hipStream_t stream = ctx->stream;
    DevBuf d_text(ctx, PT_SLOT_TEXT), d_out(ctx, PT_SLOT_OUT);
    PGX_HIP(d_text.alloc((size_t)text_bytes));
    PGX_HIP(d_out.alloc((size_t)n * 8));
    int rc = pgx_staged_h2d(ctx, d_text.p, text, (size_t)text_bytes, stream);
    if (rc != PGX_OK) return rc;
    // the loaded set: the pointers pgx_pattern_load left in the context (its slots are touched by nothing else)
    uint32_t *d_first = d_out.as<uint32_t>(), *d_count = d_first + n;
    rc = pattern_scan(ctx, d_text.as<uint8_t>(), text_bytes, static_cast<const uint8_t *>(ctx->pattern_d_blob),
                      static_cast<const u64 *>(ctx->pattern_d_offsets), n, seed, ctx->pattern_flags, ctx->pattern_d_ws, d_first,
                      d_count, stream);
    if (rc != PGX_OK) return rc;
    PGX_HIP(hipMemcpyAsync(out_first, d_first, (size_t)n * 4, hipMemcpyDeviceToHost, stream));
    PGX_HIP(hipMemcpyAsync(out_count, d_count, (size_t)n * 4, hipMemcpyDeviceToHost, stream));
    PGX_HIP(hipStreamSynchronize(stream));
    return PGX_OK;
}

}  // namespace

extern "C" {

uint32_t pgx_pattern_scan_tile(void) { return PT_TILE; }

size_t pgx_pattern_workspace_bytes(uint64_t pattern_bytes, uint32_t n_patterns) {
    if (!sizes_ok(pattern_bytes, n_patterns)) return 0;
    return make_geom(n_patterns).bytes;
}

int pgx_pattern_load(pgx_ctx *ctx, const uint8_t *patterns, const uint64_t *pattern_offsets, uint32_t n_patterns, uint32_t seed,
                     uint32_t flags) {
    return guarded(__func__, [&] { return pattern_load_host(ctx, patterns, pattern_offsets, n_patterns, seed, flags); });
}

int pgx_pattern_query(pgx_ctx *ctx, const uint8_t *text, uint64_t text_bytes, uint32_t *out_first, uint32_t *out_count) {
    return guarded(__func__, [&] { return pattern_query_host(ctx, text, text_bytes, out_first, out_count); });
}

int pgx_pattern_scan_dev(pgx_ctx *ctx, const uint8_t *d_text, uint64_t text_bytes, const uint8_t *d_patterns,
                         const uint64_t *d_pattern_offsets, uint32_t n_patterns, uint32_t seed, uint32_t flags,
                         uint32_t *d_first, uint32_t *d_count, void *d_workspace, size_t workspace_bytes, void *stream) {
    return guarded(__func__, [&] {
        return pattern_scan_dev(ctx, d_text, text_bytes, d_patterns, (const u64 *)d_pattern_offsets, n_patterns, seed, flags,
                                d_first, d_count, d_workspace, workspace_bytes, (hipStream_t)stream);
    });
}

}  // extern "C"
