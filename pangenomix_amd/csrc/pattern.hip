// Exact multi-pattern matching of variable-length patterns (the primitive behind pangenomix_amd.mlst; reference
// pangenome_analysis.py:402-453 run_mlst shells out to an external typing tool): for every pattern, WHERE it first occurs in
// the text and HOW OFTEN. Pattern k is the bytes [offsets[k], offsets[k + 1]) of a blob, L_k of them;
//   first[k] = the smallest i with text[i .. i + L_k) == pattern k, 0xFFFFFFFF for none
//   count[k] = the number of such i (overlapping occurrences each count)
// Bytes are bytes: no case folding, no alphabet; contigs and strands are the caller's business.
//
// Only the first `seed` bytes of a pattern are hashed, into text_index.h's index (its header comment has the layout; the
// payload of an entry is the pattern's index, n_patterns < 2^24), and the hash only decides WHERE to look: an occurrence is
// counted after all L_k bytes have been compared, so the result is exact whatever the hash does -- PGX_PATTERN_NARROW_HASH
// keeps 3 bits of it and must give the same output. Patterns that share a seed are a run of equal-tag entries: the normal
// case for the alleles of one locus.
//
// Kernels (plain launches on one stream):
//   pattern_build_kernel  one lane per pattern: hash of its seed, then text_index::insert_entry. A pattern shorter than the
//                         seed (the host entries refuse it) is not inserted.
//   pattern_scan_kernel   text_index::for_each_tile (a halo of seed - 1 bytes) and for_each_round: a lane hashes the seed at
//                         its position, tests the filter and walks the table ALONE up to the first tag match or an empty slot
//                         (probe_alone). Then the wave verifies together (for_each_tag_match, which has the rules every
//                         ballot and shuffle here depends on): for every equal-tag entry whose pattern fits before text_bytes
//                         the 64 lanes compare pattern and text 16 bytes per lane and 1 KiB per step (string_hash.h
//                         load_chunk: aligned 16-byte loads inside the buffers, bytes at their edges), one ballot per step
//                         ending a pattern at its first difference. Lane 0 then does atomicMin(first[k]) and
//                         atomicAdd(count[k]): a minimum and an integer sum over a set, so the same input gives the same
//                         bytes on every call.
//                         The text beyond the seed is read from global memory: a pattern may be longer than a tile.
#include "pgx_internal.h"
#include "string_hash.h"
#include "text_index.h"

namespace {

using namespace text_index;
using string_hash::Chunk;
using string_hash::load_chunk;
using string_hash::string_span;

constexpr uint32_t PT_MAX_SEED = 64;                     // the halo's maximum
constexpr uint32_t PT_TAG_SHIFT = 24;
constexpr uint32_t PT_CHUNK = 16;                        // bytes per lane and step of a comparison

bool sizes_ok(uint64_t pattern_bytes, uint32_t n_patterns) { return pattern_bytes < (1ull << 32) && n_patterns < (1u << 24); }

Geom pattern_geom(uint32_t n_patterns) { return make_geom(n_patterns, 0); }

__global__ __launch_bounds__(TI_THREADS) void pattern_build_kernel(const uint8_t *__restrict__ patterns,
                                                                   const u64 *__restrict__ offsets, uint32_t n_patterns,
                                                                   uint32_t seed, uint32_t flags, u64 *table, uint32_t mask,
                                                                   uint32_t *__restrict__ filter) {
    const uint32_t k = blockIdx.x * TI_THREADS + threadIdx.x;
    if (k >= n_patterns) return;
    u64 begin, len;
    string_span(offsets, k, offsets[n_patterns], begin, len);
    if (len < seed) return;                                  // (no seed to hash: the pattern matches nowhere)
    const u64 h = hash_bytes(patterns + begin, seed, flags & PGX_PATTERN_NARROW_HASH);
    insert_entry(table, mask, filter, h, make_entry<PT_TAG_SHIFT>(h, k));
}

__global__ __launch_bounds__(TI_THREADS) void pattern_scan_kernel(const uint8_t *__restrict__ text, uint32_t text_bytes,
                                                                  const uint8_t *__restrict__ patterns,
                                                                  const u64 *__restrict__ offsets, uint32_t n_patterns,
                                                                  uint32_t seed, uint32_t flags, const u64 *__restrict__ table,
                                                                  uint32_t mask, const uint32_t *__restrict__ filter,
                                                                  uint32_t n_tiles, uint32_t *__restrict__ first,
                                                                  uint32_t *__restrict__ count) {
    const uint32_t lane = threadIdx.x & 63u;
    const u64 total = offsets[n_patterns];
    for_each_tile<PT_MAX_SEED>(text, text_bytes, seed, filter, n_tiles,
        [&](uint32_t t0, uint32_t pos_here, const uint8_t *s_tile, const uint32_t *s_filter) {
        for_each_round(pos_here, [&](uint32_t p, bool has_position) {
            bool hit = false;
            u64 h = 0;
            if (has_position) {
                h = hash_bytes(s_tile + p, seed, flags & PGX_PATTERN_NARROW_HASH);
                hit = filter_has(s_filter, h) && probe_alone<PT_TAG_SHIFT>(table, mask, h);
            }
            for_each_tag_match<PT_TAG_SHIFT>(table, mask, hit, t0 + p, h, [&](u64 e, uint32_t gp) {
                const uint32_t k = (uint32_t)e & 0xFFFFFFu;
                u64 begin, len;
                string_span(offsets, k, total, begin, len);
                if (len < seed || (u64)gp + len > text_bytes) return;            // it would run past the text
                const u64 n_chunks = (len + PT_CHUNK - 1) / PT_CHUNK;
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
                    if (__ballot(differs)) return;
                }
                if (lane == 0u) {
                    atomicMin(&first[k], gp);
                    atomicAdd(&count[k], 1u);
                }
            });
        });
        });
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
    const Geom g = pattern_geom(n_patterns);
    PGX_HIP(enqueue_clear(d_ws, g, stream));
    {
        ProfScope prof(ctx, "pattern_build_kernel", stream);
        pattern_build_kernel<<<ceil_div_u32(n_patterns, TI_THREADS), TI_THREADS, 0, stream>>>(d_patterns, d_offsets, n_patterns,
                                                                                             seed, flags, g.table(d_ws), g.mask(),
                                                                                             g.filter(d_ws));
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
    const Geom g = pattern_geom(n_patterns);
    const uint32_t n_tiles = tiles_of(text_bytes, seed);
    {
        ProfScope prof(ctx, "pattern_scan_kernel", stream);
        pattern_scan_kernel<<<grid_of(n_tiles), TI_THREADS, 0, stream>>>(d_text, (uint32_t)text_bytes, d_patterns, d_offsets,
                                                                        n_patterns, seed, flags, g.table(d_ws), g.mask(),
                                                                        g.filter(d_ws), n_tiles, d_first, d_count);
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
    PGX_REQUIRE(d_ws && ws_bytes >= pattern_geom(n_patterns).bytes, "workspace too small (see pgx_pattern_workspace_bytes)");
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
    const char *broken = pattern_set_error(offsets, n_patterns, [&](uint32_t, uint64_t length) {
        return length >= seed ? nullptr : "a pattern is shorter than the seed";
    });
    PGX_REQUIRE(!broken, broken);
    PGX_REQUIRE(offsets[n_patterns] == 0 || patterns, "NULL patterns");
    PGX_HIP(hipSetDevice(ctx->device_id));
    ctx->pattern_loaded = false;
    DevBuf d_blob(ctx, PT_SLOT_PATTERNS), d_off(ctx, PT_SLOT_OFFSETS), d_ws(ctx, PT_SLOT_WS);
    PGX_HIP(d_ws.alloc(pattern_geom(n_patterns).bytes));
    rc = upload_pattern_set(ctx, d_blob, d_off, patterns, offsets, n_patterns);
    if (rc != PGX_OK) return rc;
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

uint32_t pgx_pattern_scan_tile(void) { return TI_TILE; }

size_t pgx_pattern_workspace_bytes(uint64_t pattern_bytes, uint32_t n_patterns) {
    if (!sizes_ok(pattern_bytes, n_patterns)) return 0;
    return pattern_geom(n_patterns).bytes;
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
