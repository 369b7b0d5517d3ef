// The seed index and the tile scan under the three text scans: scan.hip (fixed-length keys: found or not), pattern.hip
// (variable-length patterns: first occurrence and count) and near.hip (patterns within a number of mismatches). Each of them
// hashes a fixed number of bytes -- the whole key, a pattern's seed, one of a pattern's blocks -- of every entry into the
// structures below, hashes the same number of bytes at every text position, and looks the position up. The hash only decides
// WHERE to look: every scan compares bytes before it reports, so its result is exact whatever the hash does, and a scan's
// NARROW_HASH flag, which keeps 3 bits of every hash, must give the same output.
//   bits 0-17 of the hash      the entry's bit in a 2^18-bit filter (32 KiB, a copy of it sits in LDS beside the tile)
//   bits 18-...                the first slot probed in an open-addressed table of 64-bit entries, linear probing
//   bits TAG_SHIFT-63          the entry's tag; below it the entry's payload, the scan's own. TAG_SHIFT is 24 for scan.hip and
//                              pattern.hip (the index of the key or pattern: fewer than 2^24) and 32 for near.hip (a block's
//                              index above its pattern's). The low 24 bits are never all ones, so an entry is never the
//                              all-ones word that marks an empty slot.
// The table has at least twice as many slots as entries, so a probe sequence always reaches an empty slot; nothing is ever
// removed, so every entry whose hash equals a position's lies between that position's first slot and the next empty one, and
// entries that share their hashed bytes (the alleles of one locus) are a run of equal-tag entries there.
// Workspace: the table, the filter behind it, then `tail_bytes` of the scan's own that are zeroed with the filter.
//
// A scan kernel is a workgroup of TI_THREADS lanes that copies the filter to LDS and takes tiles of TI_TILE text positions:
// one tile each up to TI_MAX_GRID tiles (8 MB of text), striding beyond. Capping the grid lower was slower at 5 MB
// (profiles/window_scan_grid_caps.json). The tile and a halo of width - 1 bytes are staged in LDS (nothing at or beyond
// text_bytes is read), and lane l gets the positions l, l + 256, ... of the tile, one per round -- at every step of a hash
// consecutive lanes read consecutive bytes.
#pragma once
#include "pgx_internal.h"
#include <cassert>

namespace text_index {

typedef unsigned long long u64;

constexpr int TI_THREADS = 256;
constexpr uint32_t TI_TILE = 4096;                       // text positions per tile (pgx_*_scan_tile)
constexpr uint32_t TI_FILTER_LOG2 = 18;
constexpr uint32_t TI_FILTER_WORDS = (1u << TI_FILTER_LOG2) / 32;   // 8192 words = 32 KiB
constexpr uint32_t TI_MAX_GRID = 2048;
constexpr u64 TI_EMPTY = ~0ull;

struct Geom {
    uint32_t slots;                   // a power of two, >= 2 * n_entries
    size_t off_table, off_filter, off_tail, bytes;
    u64 *table(void *ws) const { return (u64 *)((char *)ws + off_table); }
    const u64 *table(const void *ws) const { return (const u64 *)((const char *)ws + off_table); }
    uint32_t *filter(void *ws) const { return (uint32_t *)((char *)ws + off_filter); }
    const uint32_t *filter(const void *ws) const { return (const uint32_t *)((const char *)ws + off_filter); }
    uint32_t mask() const { return slots - 1u; }
};

// n_entries < 2^30, which every caller's size check has established: `slots` has 32 bits, and the loop would not end
inline Geom make_geom(uint64_t n_entries, size_t tail_bytes) {
    assert(n_entries < (1ull << 30));
    Geom g;
    g.slots = 64;
    while (g.slots < 2 * n_entries) g.slots <<= 1;        // (at most 2^31)
    g.off_table = 0;
    g.off_filter = (size_t)g.slots * 8;                   // (a multiple of 256)
    g.off_tail = g.off_filter + (size_t)TI_FILTER_WORDS * 4;
    g.bytes = g.off_tail + tail_bytes;
    return g;
}

// every slot empty, the filter and the tail zero; enqueued on `stream`
inline hipError_t enqueue_clear(void *d_ws, const Geom &g, hipStream_t stream) {
    const hipError_t e = hipMemsetAsync(g.table(d_ws), 0xFF, (size_t)g.slots * 8, stream);
    return e != hipSuccess ? e : hipMemsetAsync(g.filter(d_ws), 0, g.bytes - g.off_filter, stream);
}

// tiles of a text that holds a `width`-byte string (text_bytes >= width), and the workgroups that take them
inline uint32_t tiles_of(uint64_t text_bytes, uint32_t width) { return (uint32_t)((text_bytes - width + 1u + TI_TILE - 1) / TI_TILE); }
inline uint32_t grid_of(uint32_t n_tiles) { return std::min(n_tiles, TI_MAX_GRID); }

struct Hash2 {
    uint32_t a = 0x9E3779B9u, b = 0x85EBCA6Bu;
    __device__ __forceinline__ void add(uint32_t byte) {
        a = a * 0x01000193u + byte + 1u;
        b = (b ^ byte) * 0x2C1B3C6Du + 0x297A2D39u;
    }
    __device__ __forceinline__ u64 value(bool narrow) const {
        u64 h = ((u64)b << 32) | a;
        h ^= h >> 33; h *= 0xFF51AFD7ED558CCDull;
        h ^= h >> 33; h *= 0xC4CEB9FE1A85EC53ull;
        h ^= h >> 33;
        return narrow ? (h & 7ull) : h;
    }
};

__device__ __forceinline__ u64 hash_bytes(const uint8_t *bytes, uint32_t n, bool narrow) {
    Hash2 hs;
    for (uint32_t j = 0; j < n; ++j) hs.add(bytes[j]);
    return hs.value(narrow);
}

__device__ __forceinline__ uint32_t filter_bit(u64 h) { return (uint32_t)h & ((1u << TI_FILTER_LOG2) - 1u); }
__device__ __forceinline__ uint32_t first_slot(u64 h, uint32_t mask) { return (uint32_t)(h >> TI_FILTER_LOG2) & mask; }
__device__ __forceinline__ bool filter_has(const uint32_t *filter, u64 h) {
    const uint32_t bit = filter_bit(h);
    return (filter[bit >> 5] >> (bit & 31u)) & 1u;
}
template <uint32_t TAG_SHIFT>
__device__ __forceinline__ u64 make_entry(u64 h, u64 payload) { return (h >> TAG_SHIFT << TAG_SHIFT) | payload; }

// A build kernel's lane: the filter bit, then the entry into the first empty slot from its hash's. The table has `mask + 1`
// >= 2 * n_entries slots, of which fewer than n_entries are taken: an empty one is always met.
__device__ __forceinline__ void insert_entry(u64 *table, uint32_t mask, uint32_t *filter, u64 h, u64 entry) {
    const uint32_t bit = filter_bit(h);
    atomicOr(&filter[bit >> 5], 1u << (bit & 31u));
    for (uint32_t s = first_slot(h, mask);; s = (s + 1u) & mask)
        if (__atomic_load_n(&table[s], __ATOMIC_RELAXED) == TI_EMPTY && atomicCAS(&table[s], TI_EMPTY, entry) == TI_EMPTY) break;
}

// A scan kernel's frame. in_tile(t0, pos_here, tile, filter) is called by the whole workgroup once per tile it takes: the
// tile's positions are t0 .. t0 + pos_here of the text, tile[p .. p + width) are the bytes of position t0 + p in LDS, `filter`
// is the copy in LDS. `in_tile` must not hold a workgroup barrier. MAX_WIDTH bounds `width` and sizes the halo: the kernel's
// static LDS is TI_TILE + MAX_WIDTH bytes and the filter.
template <uint32_t MAX_WIDTH, typename InTile>
__device__ __forceinline__ void for_each_tile(const uint8_t *__restrict__ text, uint32_t text_bytes, uint32_t width,
                                              const uint32_t *__restrict__ filter, uint32_t n_tiles, InTile in_tile) {
    constexpr uint32_t TILE_BYTES = TI_TILE + MAX_WIDTH;                         // tile + halo (width - 1 < MAX_WIDTH)
    static_assert(TILE_BYTES % 16 == 0 && TILE_BYTES + TI_FILTER_WORDS * 4 <= 64 * 1024, "static LDS stays under 64 KiB");
    __shared__ uint4 s_tile4[TILE_BYTES / 16];
    __shared__ uint4 s_filter4[TI_FILTER_WORDS / 4];
    uint8_t *s_tile = reinterpret_cast<uint8_t *>(s_tile4);
    const uint32_t *s_filter = reinterpret_cast<const uint32_t *>(s_filter4);
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < TI_FILTER_WORDS / 4; i += TI_THREADS)
        s_filter4[i] = reinterpret_cast<const uint4 *>(filter)[i];              // (the workspace is 16-byte aligned)
    const uint32_t n_pos = text_bytes - width + 1u;                              // the caller has text_bytes >= width
    const bool aligned = (reinterpret_cast<uintptr_t>(text) & 15u) == 0;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t t0 = tile * TI_TILE;                                      // < n_pos <= 2^32 - 1
        const uint32_t left = text_bytes - t0;
        const uint32_t have = left < TI_TILE + width - 1u ? left : TI_TILE + width - 1u;   // bytes staged, <= TILE_BYTES
        __syncthreads();                                                         // the tile before this one has been read
        const uint32_t whole = aligned ? have / 16u : 0u;                        // t0 is a multiple of 16
        for (uint32_t i = tid; i < whole; i += TI_THREADS)
            s_tile4[i] = reinterpret_cast<const uint4 *>(text + t0)[i];
        for (uint32_t i = whole * 16u + tid; i < have; i += TI_THREADS) s_tile[i] = text[(size_t)t0 + i];
        __syncthreads();
        in_tile(t0, n_pos - t0 < TI_TILE ? n_pos - t0 : TI_TILE, s_tile, s_filter);   // p + width <= have where p < pos_here
    }
}

// The rounds of a tile for a kernel whose waves verify together (pattern.hip, near.hip): round(p, has_position), lane l with
// p = l, l + 256, ... The number of rounds depends only on the tile, so whole waves reach `round` in every round: a lane
// whose p is past the tile's last position is told so and takes part in the ballots and shuffles there. (scan.hip's lanes
// wait for nobody and leave their loop one by one.) p is carried, not rebuilt from the round's number: written as
// r * 256 + tid the hash loop behind it had one more vector add per byte.
template <typename Round>
__device__ __forceinline__ void for_each_round(uint32_t pos_here, Round round) {
    uint32_t p = threadIdx.x;
    for (uint32_t first = 0; first < pos_here; first += TI_THREADS, p += TI_THREADS) round(p, p < pos_here);
}

// The solitary walk: does h's chain hold an entry with h's tag? It ends at the first one, so a false positive of the filter
// costs one lane a few probes.
template <uint32_t TAG_SHIFT>
__device__ __forceinline__ bool probe_alone(const u64 *__restrict__ table, uint32_t mask, u64 h) {
    const u64 tag = h >> TAG_SHIFT;
    for (uint32_t s = first_slot(h, mask);; s = (s + 1u) & mask) {
        const u64 e = table[s];
        if (e == TI_EMPTY) return false;
        if ((e >> TAG_SHIFT) == tag) return true;
    }
}

// The wave verifies together: the lanes with `hit` (position gp, hash h) are balloted and taken one at a time, position and
// hash are broadcast, and all 64 lanes walk that chain again: body(entry, position) on every equal-tag entry, with the same
// arguments on every lane, so `body` may ballot and shuffle in turn. EVERY lane of the wave must get here, in every round: a
// lane with nothing to look up comes with hit = false (its gp and h are not used). Nothing between the ballot and the end
// of the last `body` may be a workgroup barrier.
template <uint32_t TAG_SHIFT, typename Body>
__device__ __forceinline__ void for_each_tag_match(const u64 *__restrict__ table, uint32_t mask, bool hit, uint32_t gp, u64 h,
                                                   Body body) {
    u64 votes = __ballot(hit);
    while (votes) {                                                              // (the same on every lane)
        const int src = __ffsll((long long)votes) - 1;
        votes &= votes - 1ull;
        const uint32_t at = (uint32_t)__shfl((int)gp, src, 64);
        const u64 hh = ((u64)(uint32_t)__shfl((int)(uint32_t)(h >> 32), src, 64) << 32) | (uint32_t)__shfl((int)(uint32_t)h, src, 64);
        const u64 tag = hh >> TAG_SHIFT;
        for (uint32_t s = first_slot(hh, mask);; s = (s + 1u) & mask) {
            const u64 e = table[s];
            if (e == TI_EMPTY) break;
            if ((e >> TAG_SHIFT) == tag) body(e, at);
        }
    }
}

// The pattern sets of pattern.hip and near.hip: a blob and n + 1 offsets into it, as the host entries take them. The message
// of the first rule broken, or NULL: offsets non-decreasing, every length accepted by length_error(k, length) (a message or
// NULL; the caller's own rule), fewer than 2^32 bytes. `offsets` is not NULL.
template <typename LengthError>
inline const char *pattern_set_error(const uint64_t *offsets, uint32_t n_patterns, LengthError length_error) {
    for (uint32_t k = 0; k < n_patterns; ++k) {
        if (offsets[k] > offsets[k + 1]) return "offsets must not decrease";
        if (const char *msg = length_error(k, offsets[k + 1] - offsets[k])) return msg;
    }
    if (offsets[n_patterns] >= (1ull << 32)) return "a blob must hold fewer than 2^32 bytes";
    return nullptr;
}

// blob and offsets into the two slots, allocated here; the copies are enqueued on ctx->stream
inline int upload_pattern_set(pgx_ctx *ctx, DevBuf &d_blob, DevBuf &d_off, const uint8_t *patterns, const uint64_t *offsets,
                              uint32_t n_patterns) {
    const size_t bytes = (size_t)offsets[n_patterns], off_bytes = ((size_t)n_patterns + 1) * 8;
    PGX_HIP(d_blob.alloc(bytes));
    PGX_HIP(d_off.alloc(off_bytes));
    if (bytes) {
        const int rc = pgx_staged_h2d(ctx, d_blob.p, patterns, bytes, ctx->stream);
        if (rc != PGX_OK) return rc;
    }
    PGX_HIP(hipMemcpyAsync(d_off.p, offsets, off_bytes, hipMemcpyHostToDevice, ctx->stream));
    return PGX_OK;
}

}  // namespace text_index
