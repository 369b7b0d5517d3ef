// Bounded-mismatch multi-pattern matching of variable-length patterns (the primitive behind the novel-allele calls of
// pangenomix_amd.mlst): for every pattern, the full-length window of the text that differs from it in the fewest
// bytes, if that is at most max_mismatch[k] = m_k. Pattern k is the bytes [offsets[k], offsets[k + 1]) of a blob, L_k of them;
// a window of pattern k is a position i with i + L_k <= text_bytes whose L_k bytes do not hold the separator;
//   d_k(i)  = #{ j : text[i + j] != pattern_k[j] }
//   best[k] = min over windows i with d_k(i) <= m_k of (d_k(i) << 32 | i), all-ones for none or for an inactive pattern
// Bytes are bytes: no case folding, no alphabet. There is no count: a window is reached once per block that survived in it.
//
// The index is text_index.h's (its header comment has the layout), over blocks: pattern k gives its first m_k + 1
// non-overlapping blocks of `block` bytes (offsets 0, block, 2 * block, ...). m_k mismatches cannot touch m_k + 1 disjoint
// blocks, so every window within m_k holds at least one of them unchanged at its place: hashing every text position's `block`
// bytes finds it, and the distance is then counted over all L_k bytes, so the result is exact whatever the hash does --
// PGX_NEAR_NARROW_HASH keeps 3 bits of it and must give the same output. An entry's tag is 32 bits; its payload is the block's
// index (bits 24-31) above the pattern's (bits 0-23; n_patterns < 2^24).
// The table has at least twice as many slots as the n_blocks entries it is sized for, and the build kernel hands out tickets
// (the 16 bytes behind the filter): a block beyond n_blocks is not inserted, so a probe sequence always reaches an empty slot
// whatever a device caller's max_mismatch holds.
//
// Kernels (plain launches on one stream):
//   near_build_kernel  one lane per (pattern, block): workgroup k, lane j <= m_k. Hash of the block, then
//                      text_index::insert_entry. A block that does not fit its pattern is not inserted.
//   near_scan_kernel   text_index::for_each_tile (a halo of block - 1 bytes) and for_each_round: a lane hashes the block at its
//                      position, tests the filter and walks the table ALONE (probe_alone). Then the wave verifies together
//                      (for_each_tag_match, which has the rules every ballot and shuffle here depends on): every equal-tag
//                      entry (k, j) of an active pattern names the window i = position - j * block (skipped when that is
//                      before 0 or i + L_k > text_bytes). The lanes compare 16 bytes each (string_hash.h load_chunk: nothing
//                      outside [0, text_bytes) is read wherever the text starts), count their differing bytes and note a
//                      separator; one wave sum per 1 KiB step, and the window ends as soon as the sum exceeds m_k or a
//                      separator was seen. Lane 0 does a 64-bit atomicMin on best[k]: a minimum over a set, so the same input
//                      gives the same bytes on every call.
#include "pgx_internal.h"
#include "string_hash.h"
#include "text_index.h"

namespace {

using namespace text_index;
using string_hash::Chunk;
using string_hash::load_chunk;
using string_hash::string_span;

constexpr uint32_t NR_MAX_BLOCK = 64;                    // the halo's maximum
constexpr uint32_t NR_TAG_SHIFT = 32;
constexpr uint32_t NR_MAX_BLOCKS_PER_PATTERN = 256;      // m_k + 1 <= 256: one build lane each, 8 bits in an entry
constexpr size_t NR_TICKET_BYTES = 16;                   // the workspace's tail: the build kernel's ticket counter
constexpr uint32_t NR_CHUNK = 16;                        // bytes per lane and step of a comparison
constexpr u64 NR_HIGH_BITS = 0x8080808080808080ull;
constexpr uint32_t NR_SEPARATOR_SEEN = 1u << 16;         // above any sum of differing bytes of a step (64 * 16) and any m_k
static_assert(TI_THREADS == (int)NR_MAX_BLOCKS_PER_PATTERN, "the build kernel has one lane per possible block of a pattern");

bool sizes_ok(uint64_t pattern_bytes, uint32_t n_patterns, uint64_t n_blocks) {
    return pattern_bytes < (1ull << 32) && n_patterns < (1u << 24) && n_blocks < (1ull << 30);
}

Geom near_geom(uint64_t n_blocks) { return make_geom(n_blocks, NR_TICKET_BYTES); }

// bit 7 of every byte of x that is not zero
__device__ __forceinline__ u64 nonzero_bytes(u64 x) { return (((x & ~NR_HIGH_BITS) + ~NR_HIGH_BITS) | x) & NR_HIGH_BITS; }
// bit 7 of the first n (0..8) bytes
__device__ __forceinline__ u64 first_bytes(uint32_t n) { return n >= 8u ? NR_HIGH_BITS : NR_HIGH_BITS & ((1ull << (n * 8u)) - 1ull); }

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
    return v;
}

__global__ __launch_bounds__(TI_THREADS) void near_build_kernel(const uint8_t *__restrict__ patterns,
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
    const u64 h = hash_bytes(patterns + begin + (u64)j * block, block, flags & PGX_NEAR_NARROW_HASH);
    insert_entry(table, mask, filter, h, make_entry<NR_TAG_SHIFT>(h, ((u64)j << 24) | k));
}

__global__ __launch_bounds__(TI_THREADS) void near_scan_kernel(const uint8_t *__restrict__ text, uint32_t text_bytes,
                                                               uint32_t separator, const uint8_t *__restrict__ patterns,
                                                               const u64 *__restrict__ offsets, uint32_t n_patterns,
                                                               const uint8_t *__restrict__ max_mismatch,
                                                               const uint8_t *__restrict__ active, uint32_t block,
                                                               uint32_t flags, const u64 *__restrict__ table, uint32_t mask,
                                                               const uint32_t *__restrict__ filter, uint32_t n_tiles,
                                                               u64 *__restrict__ best) {
    const uint32_t lane = threadIdx.x & 63u;
    const u64 total = offsets[n_patterns];
    const bool separated = separator != PGX_NEAR_NO_SEPARATOR;
    const u64 sep8 = (u64)(separator & 0xFFu) * 0x0101010101010101ull;
    for_each_tile<NR_MAX_BLOCK>(text, text_bytes, block, filter, n_tiles,
        [&](uint32_t t0, uint32_t pos_here, const uint8_t *s_tile, const uint32_t *s_filter) {
        for_each_round(pos_here, [&](uint32_t p, bool has_position) {
            bool hit = false;
            u64 h = 0;
            if (has_position) {
                h = hash_bytes(s_tile + p, block, flags & PGX_NEAR_NARROW_HASH);
                hit = filter_has(s_filter, h) && probe_alone<NR_TAG_SHIFT>(table, mask, h);
            }
            for_each_tag_match<NR_TAG_SHIFT>(table, mask, hit, t0 + p, h, [&](u64 e, uint32_t gp) {
                const uint32_t k = (uint32_t)e & 0xFFFFFFu, j = (uint32_t)(e >> 24) & 0xFFu;
                if (k >= n_patterns || (active && !active[k])) return;
                const uint32_t behind = j * block;                               // <= 255 * 64
                if (gp < behind) return;                                         // the window would begin before the text
                const uint32_t at = gp - behind;
                u64 begin, len;
                string_span(offsets, k, total, begin, len);
                if ((u64)behind + block > len || (u64)at + len > text_bytes) return;   // it would run past the text
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
                    sum += wave_sum(mine);                                       // (the same on every lane)
                    if (sum > m) break;
                }
                if (sum <= m && lane == 0u) atomicMin(&best[k], ((u64)sum << 32) | at);
            });
        });
        });
}

int near_sizes(pgx_ctx *ctx, uint32_t n_patterns, uint32_t block, uint32_t flags) {
    PGX_REQUIRE(ctx, "NULL argument");
    PGX_REQUIRE(block >= 1 && block <= NR_MAX_BLOCK, "block must be 1..64");
    PGX_REQUIRE(n_patterns < (1u << 24), "n_patterns must be below 2^24");
    PGX_REQUIRE((flags & ~PGX_NEAR_NARROW_HASH) == 0, "unknown flags");
    return PGX_OK;
}

// table, filter and tickets of the set, enqueued on `stream`
int near_build(pgx_ctx *ctx, const uint8_t *d_patterns, const u64 *d_offsets, uint32_t n_patterns, const uint8_t *d_mm,
               uint32_t block, uint64_t n_blocks, uint32_t flags, void *d_ws, hipStream_t stream) {
    const Geom g = near_geom(n_blocks);
    PGX_HIP(enqueue_clear(d_ws, g, stream));
    {
        ProfScope prof(ctx, "near_build_kernel", stream);
        near_build_kernel<<<n_patterns, TI_THREADS, 0, stream>>>(d_patterns, d_offsets, n_patterns, d_mm, block, flags,
                                                                 g.table(d_ws), g.mask(), g.filter(d_ws),
                                                                 (uint32_t *)((char *)d_ws + g.off_tail), (uint32_t)n_blocks);
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
    const Geom g = near_geom(n_blocks);
    const uint32_t n_tiles = tiles_of(text_bytes, block);
    {
        ProfScope prof(ctx, "near_scan_kernel", stream);
        near_scan_kernel<<<grid_of(n_tiles), TI_THREADS, 0, stream>>>(d_text, (uint32_t)text_bytes, separator, d_patterns,
                                                                     d_offsets, n_patterns, d_mm, d_active, block, flags,
                                                                     g.table(d_ws), g.mask(), g.filter(d_ws), n_tiles, d_best);
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
    PGX_REQUIRE(d_ws && ws_bytes >= near_geom(n_blocks).bytes, "workspace too small (see pgx_near_workspace_bytes)");
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
    const char *broken = pattern_set_error(offsets, n_patterns, [&](uint32_t k, uint64_t length) {
        n_blocks += (uint64_t)max_mismatch[k] + 1;
        return ((uint64_t)max_mismatch[k] + 1) * block <= length ? nullptr : "a pattern is shorter than its max_mismatch + 1 blocks";
    });
    PGX_REQUIRE(!broken, broken);
    PGX_REQUIRE(n_blocks < (1ull << 30), "the patterns must give fewer than 2^30 blocks");
    PGX_REQUIRE(offsets[n_patterns] == 0 || patterns, "NULL patterns");
    PGX_HIP(hipSetDevice(ctx->device_id));
    ctx->near_loaded = false;
    DevBuf d_blob(ctx, NR_SLOT_PATTERNS), d_off(ctx, NR_SLOT_OFFSETS), d_mm(ctx, NR_SLOT_MISMATCH), d_ws(ctx, NR_SLOT_WS);
    PGX_HIP(d_mm.alloc(n_patterns));
    PGX_HIP(d_ws.alloc(near_geom(n_blocks).bytes));
    rc = upload_pattern_set(ctx, d_blob, d_off, patterns, offsets, n_patterns);
    if (rc != PGX_OK) return rc;
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

uint32_t pgx_near_scan_tile(void) { return TI_TILE; }

size_t pgx_near_workspace_bytes(uint64_t pattern_bytes, uint32_t n_patterns, uint64_t n_blocks) {
    if (!sizes_ok(pattern_bytes, n_patterns, n_blocks)) return 0;
    return near_geom(n_blocks).bytes;
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
