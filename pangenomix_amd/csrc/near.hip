// Bounded-mismatch multi-pattern matching of variable-length patterns (the primitive behind the novel-allele calls of
// pangenomix_amd.mlst): for every pattern, the full-length window of the text that differs from it in the fewest
// bytes, if that is at most max_mismatch[k] = m_k. Pattern k is the bytes [offsets[k], offsets[k + 1]) of a blob, L_k of them;
// a window of pattern k is a position i with i + L_k <= text_bytes whose L_k bytes do not hold the separator;
//   d_k(i)  = #{ j : text[i + j] != pattern_k[j] }
//   best[k] = min over windows i with d_k(i) <= m_k of (d_k(i) << 32 | i), all-ones for none or for an inactive pattern
// Bytes are bytes: no case folding, no alphabet. There is no count: a window is reached once per block that survived in it.
//
// The index is pattern.hip's, over blocks instead of seeds: pattern k gives its first m_k + 1 non-overlapping blocks of
// `block` bytes (offsets 0, block, 2 * block, ...). m_k mismatches cannot touch m_k + 1 disjoint blocks, so every window
// within m_k holds at least one of them unchanged at its place: hashing every text position's `block` bytes finds it, and the
// distance is then counted over all L_k bytes, so the result is exact whatever the hash does -- PGX_NEAR_NARROW_HASH keeps 3
// bits of it and must give the same output.
//   bits 0-17 of the hash    the block's bit in a 2^18-bit filter (32 KiB, a copy of it sits in LDS beside the tile)
//   bits 18-...              the first slot probed in an open-addressed table of 64-bit entries, linear probing
//   bits 32-63               the entry's tag; below it the block's index (bits 24-31) and the pattern's (bits 0-23; n_patterns <
//                            2^24, so an entry is never the all-ones word that marks an empty slot)
// The table has at least twice as many slots as the n_blocks entries it is sized for, and the build kernel hands out tickets:
// a block beyond n_blocks is not inserted, so a probe sequence always reaches an empty slot whatever a device caller's
// max_mismatch holds.
//
// Kernels (plain launches on one stream):
//   near_build_kernel  one lane per (pattern, block): workgroup k, lane j <= m_k. Hash of the block, atomicOr of the filter bit,
//                      insertion with atomicCAS on the first empty slot. A block that does not fit its pattern is not inserted.
//   near_scan_kernel   pattern_scan_kernel's tile, halo (block - 1 bytes) and filter staging. Lane l hashes the blocks at
//                      positions l, l + 256, ..., tests the filter and walks the table ALONE up to the first tag match or an
//                      empty slot. Then the wave verifies together: hit lanes are balloted and taken one at a time, all 64 lanes
//                      walk that chain again, and every equal-tag entry (k, j) of an active pattern names the window
//                      i = position - j * block (skipped when that is before 0 or i + L_k > text_bytes). The lanes compare 16
//                      bytes each (string_hash.h load_chunk: nothing outside [0, text_bytes) is read wherever the text
//                      starts), count their differing bytes and note a separator; one wave sum per 1 KiB step, and the window
//                      ends as soon as the sum exceeds m_k or a separator was seen. Lane 0 does a 64-bit atomicMin on best[k]:
//                      a minimum over a set, so the same input gives the same bytes on every call.
//                      Every lane of a wave reaches every ballot and shuffle: a lane with no position left takes part with "no
//                      hit", and nothing between the ballot and the end of the verification is a workgroup barrier.
#include "pgx_internal.h"
#include "string_hash.h"

namespace {

using string_hash::Chunk;
using string_hash::load_chunk;
using string_hash::string_span;
typedef unsigned long long u64;

constexpr int NR_THREADS = 256;
constexpr uint32_t NR_TILE = 4096;                       // text positions per tile (pgx_near_scan_tile)
constexpr uint32_t NR_MAX_BLOCK = 64;
constexpr uint32_t NR_MAX_BLOCKS_PER_PATTERN = 256;      // m_k + 1 <= 256: one build lane each, 8 bits in an entry
constexpr uint32_t NR_TILE_BYTES = NR_TILE + NR_MAX_BLOCK;          // tile + halo (block - 1 <= 63), a multiple of 16
constexpr uint32_t NR_FILTER_LOG2 = 18;
constexpr uint32_t NR_FILTER_WORDS = (1u << NR_FILTER_LOG2) / 32;   // 8192 words = 32 KiB
constexpr uint32_t NR_MAX_GRID = 2048;
constexpr uint32_t NR_CHUNK = 16;                        // bytes per lane and step of a comparison
constexpr u64 NR_EMPTY = ~0ull;
constexpr u64 NR_HIGH_BITS = 0x8080808080808080ull;
constexpr uint32_t NR_SEPARATOR_SEEN = 1u << 16;         // above any sum of differing bytes of a step (64 * 16) and any m_k
static_assert(NR_TILE_BYTES % 16 == 0 && NR_TILE_BYTES + NR_FILTER_WORDS * 4 <= 64 * 1024, "static LDS stays under 64 KiB");
static_assert(NR_THREADS == (int)NR_MAX_BLOCKS_PER_PATTERN, "the build kernel has one lane per possible block of a pattern");

struct NearGeom {
    uint32_t slots;                   // a power of two, >= 2 * n_blocks
    size_t off_table, off_filter, off_tickets, bytes;
};

bool sizes_ok(uint64_t pattern_bytes, uint32_t n_patterns, uint64_t n_blocks) {
    return pattern_bytes < (1ull << 32) && n_patterns < (1u << 24) && n_blocks < (1ull << 30);
}

NearGeom make_geom(uint64_t n_blocks) {
    NearGeom g;
    g.slots = 64;
    while (g.slots < 2 * n_blocks) g.slots <<= 1;         // (n_blocks < 2^30: at most 2^31)
    g.off_table = 0;
    g.off_filter = (size_t)g.slots * 8;                   // (a multiple of 256)
    g.off_tickets = g.off_filter + (size_t)NR_FILTER_WORDS * 4;
    g.bytes = g.off_tickets + 16;
    return g;
}

// scan.hip's hash and slot helpers, restated (its kernels and pattern.hip's stay as they are)
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
        return (flags & PGX_NEAR_NARROW_HASH) ? (h & 7ull) : h;
    }
};

__device__ __forceinline__ uint32_t filter_bit(u64 h) { return (uint32_t)h & ((1u << NR_FILTER_LOG2) - 1u); }
__device__ __forceinline__ uint32_t first_slot(u64 h, uint32_t mask) { return (uint32_t)(h >> NR_FILTER_LOG2) & mask; }
__device__ __forceinline__ uint32_t tag_of(u64 h) { return (uint32_t)(h >> 32); }

// bit 7 of every byte of x that is not zero
__device__ __forceinline__ u64 nonzero_bytes(u64 x) { return (((x & ~NR_HIGH_BITS) + ~NR_HIGH_BITS) | x) & NR_HIGH_BITS; }
// bit 7 of the first n (0..8) bytes
__device__ __forceinline__ u64 first_bytes(uint32_t n) { return n >= 8u ? NR_HIGH_BITS : NR_HIGH_BITS & ((1ull << (n * 8u)) - 1ull); }

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
    return v;
}

__global__ __launch_bounds__(NR_THREADS) void near_build_kernel(const uint8_t *__restrict__ patterns,
                                                                const u64 *__restrict__ offsets, uint32_t n_patterns,
                                                                const uint8_t *__restrict__ max_mismatch, uint32_t block,
                                                                uint32_t flags, u64 *table, uint32_t mask,
                                                                uint32_t *__restrict__ filter, uint32_t *tickets,
                                                                uint32_t n_blocks) {
    const uint32_t k = blockIdx.x, j = threadIdx.x;
    if (k >= n_patterns || j > max_mismatch[k]) return;
    u64 begin, len;
    string_span(offsets, k, offsets[n_patterns], begin, len);
    if ((u64)(j + 1u) * block > len) return;                 // (the block does not fit: the host entries refuse the pattern)
    if (atomicAdd(tickets, 1u) >= n_blocks) return;          // (more blocks than the table was sized for)
    Hash2 hs;
    for (uint32_t b = 0; b < block; ++b) hs.add(patterns[begin + (u64)j * block + b]);
    const u64 h = hs.value(flags);
    const uint32_t bit = filter_bit(h);
    atomicOr(&filter[bit >> 5], 1u << (bit & 31u));
    const u64 entry = ((u64)tag_of(h) << 32) | ((u64)j << 24) | k;
    uint32_t s = first_slot(h, mask);
    // `mask + 1` >= 2 * n_blocks slots, of which fewer than n_blocks are taken: an empty one is always met
    for (;;) {
        if (__atomic_load_n(&table[s], __ATOMIC_RELAXED) == NR_EMPTY && atomicCAS(&table[s], NR_EMPTY, entry) == NR_EMPTY)
            break;
        s = (s + 1u) & mask;
    }
}

__global__ __launch_bounds__(NR_THREADS) void near_scan_kernel(const uint8_t *__restrict__ text, uint32_t text_bytes,
                                                               uint32_t separator, const uint8_t *__restrict__ patterns,
                                                               const u64 *__restrict__ offsets, uint32_t n_patterns,
                                                               const uint8_t *__restrict__ max_mismatch,
                                                               const uint8_t *__restrict__ active, uint32_t block,
                                                               uint32_t flags, const u64 *__restrict__ table, uint32_t mask,
                                                               const uint32_t *__restrict__ filter, uint32_t n_tiles,
                                                               u64 *__restrict__ best) {
    __shared__ uint4 s_tile4[NR_TILE_BYTES / 16];
    __shared__ uint4 s_filter4[NR_FILTER_WORDS / 4];
    uint8_t *s_tile = reinterpret_cast<uint8_t *>(s_tile4);
    const uint32_t *s_filter = reinterpret_cast<const uint32_t *>(s_filter4);
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    for (uint32_t i = tid; i < NR_FILTER_WORDS / 4; i += NR_THREADS)
        s_filter4[i] = reinterpret_cast<const uint4 *>(filter)[i];              // (the workspace is 16-byte aligned)
    const u64 total = offsets[n_patterns];
    const uint32_t n_pos = text_bytes - block + 1u;                              // the caller has text_bytes >= block
    const bool aligned = (reinterpret_cast<uintptr_t>(text) & 15u) == 0;
    const bool separated = separator != PGX_NEAR_NO_SEPARATOR;
    const u64 sep8 = (u64)(separator & 0xFFu) * 0x0101010101010101ull;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t t0 = tile * NR_TILE;                                      // < n_pos <= 2^32 - 1
        const uint32_t left = text_bytes - t0;
        const uint32_t have = left < NR_TILE + block - 1u ? left : NR_TILE + block - 1u;   // bytes staged, <= NR_TILE_BYTES
        __syncthreads();                                                         // the tile before this one has been read
        const uint32_t whole = aligned ? have / 16u : 0u;                        // t0 is a multiple of 16
        for (uint32_t i = tid; i < whole; i += NR_THREADS)
            s_tile4[i] = reinterpret_cast<const uint4 *>(text + t0)[i];
        for (uint32_t i = whole * 16u + tid; i < have; i += NR_THREADS) s_tile[i] = text[(size_t)t0 + i];
        __syncthreads();
        const uint32_t pos_here = n_pos - t0 < NR_TILE ? n_pos - t0 : NR_TILE;
        // r and pos_here are the same on every lane of the workgroup: whole waves take every round, a lane without a
        // position votes "no hit"
        for (uint32_t r = 0; r * NR_THREADS < pos_here; ++r) {
            const uint32_t p = r * NR_THREADS + tid;                             // p + block <= have where p < pos_here
            bool hit = false;
            u64 h = 0;
            if (p < pos_here) {
                Hash2 hs;
                for (uint32_t j = 0; j < block; ++j) hs.add(s_tile[p + j]);
                h = hs.value(flags);
                const uint32_t bit = filter_bit(h);
                if ((s_filter[bit >> 5] >> (bit & 31u)) & 1u) {
                    const uint32_t tag = tag_of(h);
                    for (uint32_t s = first_slot(h, mask);; s = (s + 1u) & mask) {
                        const u64 e = table[s];
                        if (e == NR_EMPTY) break;
                        if ((uint32_t)(e >> 32) == tag) { hit = true; break; }
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
                const uint32_t tag = tag_of(hh);
                for (uint32_t s = first_slot(hh, mask);; s = (s + 1u) & mask) {
                    const u64 e = table[s];
                    if (e == NR_EMPTY) break;
                    if ((uint32_t)(e >> 32) != tag) continue;
                    const uint32_t k = (uint32_t)e & 0xFFFFFFu, j = (uint32_t)(e >> 24) & 0xFFu;
                    if (k >= n_patterns || (active && !active[k])) continue;
                    const uint32_t behind = j * block;                           // <= 255 * 64
                    if (gp < behind) continue;                                   // the window would begin before the text
                    const uint32_t at = gp - behind;
                    u64 begin, len;
                    string_span(offsets, k, total, begin, len);
                    if ((u64)behind + block > len || (u64)at + len > text_bytes) continue;   // it would run past the text
                    const uint32_t m = max_mismatch[k];
                    const u64 n_chunks = (len + NR_CHUNK - 1) / NR_CHUNK;
                    uint32_t sum = 0;
                    for (u64 base = 0; base < n_chunks; base += 64) {
                        const u64 c = base + lane;
                        uint32_t mine = 0;
                        if (c < n_chunks) {
                            const u64 rest = len - c * NR_CHUNK;
                            const uint32_t n = rest < NR_CHUNK ? (uint32_t)rest : NR_CHUNK;
                            const Chunk a = load_chunk(patterns, total, begin + c * NR_CHUNK, n);
                            const Chunk b = load_chunk(text, text_bytes, (u64)at + c * NR_CHUNK, n);
                            // (bytes n.. are zero in both)
                            mine = (uint32_t)__popcll(nonzero_bytes(a.lo ^ b.lo)) + (uint32_t)__popcll(nonzero_bytes(a.hi ^ b.hi));
                            if (separated) {
                                const u64 lo = first_bytes(n < 8u ? n : 8u), hi = first_bytes(n < 8u ? 0u : n - 8u);
                                if ((nonzero_bytes(b.lo ^ sep8) & lo) != lo || (nonzero_bytes(b.hi ^ sep8) & hi) != hi)
                                    mine += NR_SEPARATOR_SEEN;
                            }
                        }
                        sum += wave_sum(mine);                                   // (the same on every lane)
                        if (sum > m) break;
                    }
                    if (sum <= m && lane == 0u) atomicMin(&best[k], ((u64)sum << 32) | at);
                }
            }
        }
    }
}

int near_sizes(pgx_ctx *ctx, uint32_t n_patterns, uint32_t block, uint32_t flags) {
    PGX_REQUIRE(ctx, "NULL argument");
    PGX_REQUIRE(block >= 1 && block <= NR_MAX_BLOCK, "block must be 1..64");
    PGX_REQUIRE(n_patterns < (1u << 24), "n_patterns must be below 2^24");
    PGX_REQUIRE((flags & ~PGX_NEAR_NARROW_HASH) == 0, "unknown flags");
    return PGX_OK;
}

// table and filter of the set, enqueued on `stream`
int near_build(pgx_ctx *ctx, const uint8_t *d_patterns, const u64 *d_offsets, uint32_t n_patterns, const uint8_t *d_mm,
               uint32_t block, uint64_t n_blocks, uint32_t flags, void *d_ws, hipStream_t stream) {
    const NearGeom g = make_geom(n_blocks);
    u64 *table = (u64 *)((char *)d_ws + g.off_table);
    uint32_t *filter = (uint32_t *)((char *)d_ws + g.off_filter);
    uint32_t *tickets = (uint32_t *)((char *)d_ws + g.off_tickets);
    PGX_HIP(hipMemsetAsync(table, 0xFF, (size_t)g.slots * 8, stream));
    PGX_HIP(hipMemsetAsync(filter, 0, (size_t)NR_FILTER_WORDS * 4 + 16, stream));           // (and the tickets behind it)
    {
        ProfScope prof(ctx, "near_build_kernel", stream);
        near_build_kernel<<<n_patterns, NR_THREADS, 0, stream>>>(d_patterns, d_offsets, n_patterns, d_mm, block, flags, table,
                                                                 g.slots - 1u, filter, tickets, (uint32_t)n_blocks);
    }
    PGX_HIP(hipGetLastError());
    return PGX_OK;
}

// best = all-ones, then the scan where the text holds a block; enqueued on `stream`. n_patterns >= 1.
int near_scan(pgx_ctx *ctx, const uint8_t *d_text, uint64_t text_bytes, uint32_t separator, const uint8_t *d_patterns,
              const u64 *d_offsets, uint32_t n_patterns, const uint8_t *d_mm, const uint8_t *d_active, uint32_t block,
              uint64_t n_blocks, uint32_t flags, const void *d_ws, u64 *d_best, hipStream_t stream) {
    PGX_HIP(hipMemsetAsync(d_best, 0xFF, (size_t)n_patterns * 8, stream));
    if (text_bytes < block) return PGX_OK;
    const NearGeom g = make_geom(n_blocks);
    const u64 *table = (const u64 *)((const char *)d_ws + g.off_table);
    const uint32_t *filter = (const uint32_t *)((const char *)d_ws + g.off_filter);
    const uint64_t n_pos = text_bytes - block + 1u;
    const uint32_t n_tiles = (uint32_t)((n_pos + NR_TILE - 1) / NR_TILE);
    {
        ProfScope prof(ctx, "near_scan_kernel", stream);
        near_scan_kernel<<<std::min(n_tiles, NR_MAX_GRID), NR_THREADS, 0, stream>>>(d_text, (uint32_t)text_bytes, separator,
                                                                                   d_patterns, d_offsets, n_patterns, d_mm,
                                                                                   d_active, block, flags, table, g.slots - 1u,
                                                                                   filter, n_tiles, d_best);
    }
    PGX_HIP(hipGetLastError());
    return PGX_OK;
}

// Everything on the device; `stream` is synchronised once, at the end.
int near_scan_dev(pgx_ctx *ctx, const uint8_t *d_text, uint64_t text_bytes, uint32_t separator, const uint8_t *d_patterns,
                  const u64 *d_offsets, uint32_t n_patterns, const uint8_t *d_mm, uint32_t block, uint64_t n_blocks,
                  uint32_t flags, const uint8_t *d_active, u64 *d_best, void *d_ws, size_t ws_bytes, hipStream_t stream) {
    int rc = near_sizes(ctx, n_patterns, block, flags);
    if (rc != PGX_OK) return rc;
    PGX_REQUIRE(text_bytes < (1ull << 32), "text_bytes must be below 2^32");
    PGX_REQUIRE(separator <= PGX_NEAR_NO_SEPARATOR, "separator must be a byte value or PGX_NEAR_NO_SEPARATOR");
    PGX_REQUIRE(n_blocks < (1ull << 30), "n_blocks must be below 2^30");
    if (n_patterns == 0) return PGX_OK;
    PGX_REQUIRE(d_patterns && d_offsets && d_mm && d_best, "NULL patterns, offsets, max_mismatch or best");
    PGX_REQUIRE(text_bytes == 0 || d_text, "NULL text");
    PGX_REQUIRE(((uintptr_t)d_offsets & 7u) == 0 && ((uintptr_t)d_best & 7u) == 0, "offsets and best must be 8-byte aligned");
    PGX_REQUIRE(d_ws && ws_bytes >= make_geom(n_blocks).bytes, "workspace too small (see pgx_near_workspace_bytes)");
    PGX_REQUIRE(((uintptr_t)d_ws & 15u) == 0, "workspace must be 16-byte aligned");
    if (text_bytes >= block) {
        rc = near_build(ctx, d_patterns, d_offsets, n_patterns, d_mm, block, n_blocks, flags, d_ws, stream);
        if (rc != PGX_OK) return rc;
    }
    rc = near_scan(ctx, d_text, text_bytes, separator, d_patterns, d_offsets, n_patterns, d_mm, d_active, block, n_blocks, flags,
                   d_ws, d_best, stream);
    if (rc != PGX_OK) return rc;
    PGX_HIP(hipStreamSynchronize(stream));
    return PGX_OK;
}

int near_load_host(pgx_ctx *ctx, const uint8_t *patterns, const uint64_t *offsets, uint32_t n_patterns,
                   const uint8_t *max_mismatch, uint32_t block, uint32_t flags) {
    int rc = near_sizes(ctx, n_patterns, block, flags);
    if (rc != PGX_OK) return rc;
    PGX_REQUIRE(offsets, "NULL pattern_offsets");
    PGX_REQUIRE(n_patterns == 0 || max_mismatch, "NULL max_mismatch");
    uint64_t n_blocks = 0;
    for (uint32_t k = 0; k < n_patterns; ++k) {
        PGX_REQUIRE(offsets[k] <= offsets[k + 1], "offsets must not decrease");
        PGX_REQUIRE(((uint64_t)max_mismatch[k] + 1) * block <= offsets[k + 1] - offsets[k],
                    "a pattern is shorter than its max_mismatch + 1 blocks");
        n_blocks += (uint64_t)max_mismatch[k] + 1;
    }
    PGX_REQUIRE(offsets[n_patterns] < (1ull << 32), "a blob must hold fewer than 2^32 bytes");
    PGX_REQUIRE(n_blocks < (1ull << 30), "the patterns must give fewer than 2^30 blocks");
    PGX_REQUIRE(offsets[n_patterns] == 0 || patterns, "NULL patterns");
    PGX_HIP(hipSetDevice(ctx->device_id));
    ctx->near_loaded = false;
    const size_t bytes = (size_t)offsets[n_patterns];
    DevBuf d_blob(ctx, NR_SLOT_PATTERNS), d_off(ctx, NR_SLOT_OFFSETS), d_mm(ctx, NR_SLOT_MISMATCH), d_ws(ctx, NR_SLOT_WS);
    PGX_HIP(d_blob.alloc(bytes));
    PGX_HIP(d_off.alloc(((size_t)n_patterns + 1) * 8));
    PGX_HIP(d_mm.alloc(n_patterns));
    PGX_HIP(d_ws.alloc(make_geom(n_blocks).bytes));
    if (bytes) {
        rc = pgx_staged_h2d(ctx, d_blob.p, patterns, bytes, ctx->stream);
        if (rc != PGX_OK) return rc;
    }
    PGX_HIP(hipMemcpyAsync(d_off.p, offsets, ((size_t)n_patterns + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    if (n_patterns) {
        PGX_HIP(hipMemcpyAsync(d_mm.p, max_mismatch, n_patterns, hipMemcpyHostToDevice, ctx->stream));
        rc = near_build(ctx, d_blob.as<uint8_t>(), d_off.as<u64>(), n_patterns, d_mm.as<uint8_t>(), block, n_blocks, flags,
                        d_ws.p, ctx->stream);
        if (rc != PGX_OK) return rc;
    }
    PGX_HIP(hipStreamSynchronize(ctx->stream));
    ctx->near_loaded = true;
    ctx->near_count = n_patterns;
    ctx->near_block = block;
    ctx->near_flags = flags;
    ctx->near_blocks = n_blocks;
    ctx->near_d_blob = d_blob.p;
    ctx->near_d_offsets = d_off.p;
    ctx->near_d_mismatch = d_mm.p;
    ctx->near_d_ws = d_ws.p;
    return PGX_OK;
}

int near_query_host(pgx_ctx *ctx, const uint8_t *text, uint64_t text_bytes, uint32_t separator, const uint8_t *active,
                    uint64_t *out_best) {
    PGX_REQUIRE(ctx, "NULL argument");
    PGX_REQUIRE(ctx->near_loaded, "no set of patterns is loaded (pgx_near_load)");
    PGX_REQUIRE(text_bytes < (1ull << 32), "text_bytes must be below 2^32");
    PGX_REQUIRE(separator <= PGX_NEAR_NO_SEPARATOR, "separator must be a byte value or PGX_NEAR_NO_SEPARATOR");
    const uint32_t n = ctx->near_count, block = ctx->near_block;
    if (n == 0) return PGX_OK;
    PGX_REQUIRE(out_best, "NULL out_best");
    PGX_REQUIRE(text_bytes == 0 || text, "NULL text");
    if (text_bytes < block) {                                                    // no block: nothing to upload
        memset(out_best, 0xFF, (size_t)n * 8);
        return PGX_OK;
    }
    PGX_HIP(hipSetDevice(ctx->device_id));
    hipStream_t stream = ctx->stream;
    DevBuf d_text(ctx, NR_SLOT_TEXT), d_active(ctx, NR_SLOT_ACTIVE), d_out(ctx, NR_SLOT_OUT);
    PGX_HIP(d_text.alloc((size_t)text_bytes));
    PGX_HIP(d_active.alloc(n));
    PGX_HIP(d_out.alloc((size_t)n * 8));
    int rc = pgx_staged_h2d(ctx, d_text.p, text, (size_t)text_bytes, stream);
    if (rc != PGX_OK) return rc;
    if (active) PGX_HIP(hipMemcpyAsync(d_active.p, active, n, hipMemcpyHostToDevice, stream));
    // the loaded set: the pointers pgx_near_load left in the context (its slots are touched by nothing else)
    rc = near_scan(ctx, d_text.as<uint8_t>(), text_bytes, separator, static_cast<const uint8_t *>(ctx->near_d_blob),
                   static_cast<const u64 *>(ctx->near_d_offsets), n, static_cast<const uint8_t *>(ctx->near_d_mismatch),
                   active ? d_active.as<uint8_t>() : nullptr, block, ctx->near_blocks, ctx->near_flags, ctx->near_d_ws,
                   d_out.as<u64>(), stream);
    if (rc != PGX_OK) return rc;
    PGX_HIP(hipMemcpyAsync(out_best, d_out.p, (size_t)n * 8, hipMemcpyDeviceToHost, stream));
    PGX_HIP(hipStreamSynchronize(stream));
    return PGX_OK;
}

}  // namespace

extern "C" {

uint32_t pgx_near_scan_tile(void) { return NR_TILE; }

size_t pgx_near_workspace_bytes(uint64_t pattern_bytes, uint32_t n_patterns, uint64_t n_blocks) {
    if (!sizes_ok(pattern_bytes, n_patterns, n_blocks)) return 0;
    return make_geom(n_blocks).bytes;
}

int pgx_near_load(pgx_ctx *ctx, const uint8_t *patterns, const uint64_t *pattern_offsets, uint32_t n_patterns,
                  const uint8_t *max_mismatch, uint32_t block, uint32_t flags) {
    return guarded(__func__, [&] { return near_load_host(ctx, patterns, pattern_offsets, n_patterns, max_mismatch, block, flags); });
}

int pgx_near_query(pgx_ctx *ctx, const uint8_t *text, uint64_t text_bytes, uint32_t separator, const uint8_t *active,
                   uint64_t *out_best) {
    return guarded(__func__, [&] { return near_query_host(ctx, text, text_bytes, separator, active, out_best); });
}

int pgx_near_scan_dev(pgx_ctx *ctx, const uint8_t *d_text, uint64_t text_bytes, uint32_t separator, const uint8_t *d_patterns,
                      const uint64_t *d_pattern_offsets, uint32_t n_patterns, const uint8_t *d_max_mismatch, uint32_t block,
                      uint64_t n_blocks, uint32_t flags, const uint8_t *d_active, uint64_t *d_best, void *d_workspace,
                      size_t workspace_bytes, void *stream) {
    return guarded(__func__, [&] {
        return near_scan_dev(ctx, d_text, text_bytes, separator, d_patterns, (const u64 *)d_pattern_offsets, n_patterns,
                             d_max_mismatch, block, n_blocks, flags, d_active, (u64 *)d_best, d_workspace, workspace_bytes,
                             (hipStream_t)stream);
    });
}

}  // extern "C"
