// Exact multi-pattern matching of fixed-length keys (reference pangenome.py:1573-1647 validate_proximal_table_direct slides a
// window over every contig, one dict look-up per base): found[k] = 1 iff the `window` bytes of key k occur anywhere in the
// text. Bytes are bytes: no case folding, no alphabet; contigs and strands are the caller's business (pangenome.py joins the
// contigs with a byte no key holds and adds the reverse complements of the KEYS).
//
// Every window-long string is hashed to 64 bits (two 32-bit polynomial hashes, mixed). The hash only decides WHERE to look:
// a key is reported only after its bytes have been compared with the text's, so the result is exact whatever the hash does
// -- PGX_SCAN_NARROW_HASH keeps 3 bits of it and must give the same output.
//   bits 0-17 of the hash    the key's bit in a 2^18-bit filter (32 KiB, a copy of it sits in LDS beside the tile)
//   bits 18-...              the first slot probed in an open-addressed table of 64-bit entries, linear probing
//   bits 24-63               the entry's 40-bit tag; its low 24 bits are the key's index (n_keys < 2^24, so an entry is never
//                            the all-ones word that marks an empty slot)
// The table has at least twice as many slots as keys, so a probe sequence always reaches an empty slot; nothing is ever
// removed, so every key whose hash equals a window's lies between that window's first slot and the next empty one.
//
// Kernels (plain launches on one stream; the only atomics are the build kernel's CAS on a slot and OR on a filter word):
//   scan_build_kernel   one lane per key: hash, atomicOr of the filter bit, insertion with atomicCAS on the first empty slot
//   scan_kernel         a workgroup copies the filter to LDS, then takes tiles of SC_TILE text positions: one tile each up to
//                       SC_MAX_GRID tiles (8 MB of text), striding beyond. Capping the grid lower was slower at 5 MB
//                       (profiles/window_scan_grid_caps.json). The tile and a halo of window - 1 bytes are staged in LDS
//                       (nothing at or beyond text_bytes is read), lane l hashes the windows at positions l, l + 256, ...
//                       -- at every step consecutive lanes read consecutive bytes -- tests the filter, and only on a hit
//                       walks the table; only on a tag match are the window's bytes compared with the key's. Equal windows
//                       store found[k] = 1: every writer writes the same value. The walk goes on past a match to the next
//                       empty slot, so equal keys are all flagged.
#include "pgx_internal.h"

namespace {

constexpr int SC_THREADS = 256;
constexpr uint32_t SC_TILE = 4096;                       // text positions per tile (pgx_window_scan_tile)
constexpr uint32_t SC_MAX_WINDOW = 1024;
constexpr uint32_t SC_PER_LANE = SC_TILE / SC_THREADS;
constexpr uint32_t SC_TILE_BYTES = SC_TILE + SC_MAX_WINDOW;          // tile + halo (window - 1 <= 1023), a multiple of 16
constexpr uint32_t SC_FILTER_LOG2 = 18;
constexpr uint32_t SC_FILTER_WORDS = (1u << SC_FILTER_LOG2) / 32;    // 8192 words = 32 KiB
constexpr uint32_t SC_MAX_GRID = 2048;
constexpr unsigned long long SC_EMPTY = ~0ull;
static_assert(SC_TILE_BYTES % 16 == 0 && SC_TILE_BYTES + SC_FILTER_WORDS * 4 <= 64 * 1024, "static LDS stays under 64 KiB");

struct ScanGeom {
    uint32_t slots;                   // a power of two, >= 2 * n_keys
    size_t off_table, off_filter, bytes;
};

bool sizes_ok(uint64_t text_bytes, uint32_t n_keys, uint32_t window) {
    return window >= 1 && window <= SC_MAX_WINDOW && text_bytes < (1ull << 32) && n_keys < (1u << 24);
}

ScanGeom make_geom(uint32_t n_keys) {
    ScanGeom g;
    g.slots = 64;
    while (g.slots < 2 * n_keys) g.slots <<= 1;           // (n_keys < 2^24: at most 2^25)
    g.off_table = 0;
    g.off_filter = (size_t)g.slots * 8;                   // (a multiple of 256)
    g.bytes = g.off_filter + (size_t)SC_FILTER_WORDS * 4;
    return g;
}

struct Hash2 {
    uint32_t a = 0x9E3779B9u, b = 0x85EBCA6Bu;
    __device__ __forceinline__ void add(uint32_t byte) {
        a = a * 0x01000193u + byte + 1u;
        b = (b ^ byte) * 0x2C1B3C6Du + 0x297A2D39u;
    }
    __device__ __forceinline__ unsigned long long value(uint32_t flags) const {
        unsigned long long h = ((unsigned long long)b << 32) | a;
        h ^= h >> 33; h *= 0xFF51AFD7ED558CCDull;
        h ^= h >> 33; h *= 0xC4CEB9FE1A85EC53ull;
        h ^= h >> 33;
        return (flags & PGX_SCAN_NARROW_HASH) ? (h & 7ull) : h;
    }
};

__device__ __forceinline__ uint32_t filter_bit(unsigned long long h) { return (uint32_t)h & ((1u << SC_FILTER_LOG2) - 1u); }
__device__ __forceinline__ uint32_t first_slot(unsigned long long h, uint32_t mask) {
    return (uint32_t)(h >> SC_FILTER_LOG2) & mask;
}
__device__ __forceinline__ unsigned long long tag_of(unsigned long long h) { return h >> 24; }

__global__ __launch_bounds__(SC_THREADS) void scan_build_kernel(const uint8_t *__restrict__ keys, uint32_t n_keys,
                                                                uint32_t window, uint32_t flags,
                                                                unsigned long long *table, uint32_t mask,
                                                                uint32_t *__restrict__ filter) {
    const uint32_t k = blockIdx.x * SC_THREADS + threadIdx.x;
    if (k >= n_keys) return;
    const uint8_t *key = keys + (size_t)k * window;
    Hash2 hs;
    for (uint32_t j = 0; j < window; ++j) hs.add(key[j]);
    const unsigned long long h = hs.value(flags);
    const uint32_t bit = filter_bit(h);
    atomicOr(&filter[bit >> 5], 1u << (bit & 31u));
    const unsigned long long entry = (tag_of(h) << 24) | k;
    uint32_t s = first_slot(h, mask);
    // at most `mask + 1` >= 2 * n_keys slots, of which fewer than n_keys are taken: an empty one is always met
    for (;;) {
        if (__atomic_load_n(&table[s], __ATOMIC_RELAXED) == SC_EMPTY && atomicCAS(&table[s], SC_EMPTY, entry) == SC_EMPTY)
            break;
        s = (s + 1u) & mask;
    }
}

__global__ __launch_bounds__(SC_THREADS) void scan_kernel(const uint8_t *__restrict__ text, uint32_t text_bytes,
                                                          const uint8_t *__restrict__ keys, uint32_t window, uint32_t flags,
                                                          const unsigned long long *__restrict__ table, uint32_t mask,
                                                          const uint32_t *__restrict__ filter, uint32_t n_tiles,
                                                          uint8_t *__restrict__ found) {
    __shared__ uint4 s_tile4[SC_TILE_BYTES / 16];
    __shared__ uint4 s_filter4[SC_FILTER_WORDS / 4];
    uint8_t *s_tile = reinterpret_cast<uint8_t *>(s_tile4);
    const uint32_t *s_filter = reinterpret_cast<const uint32_t *>(s_filter4);
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < SC_FILTER_WORDS / 4; i += SC_THREADS)
        s_filter4[i] = reinterpret_cast<const uint4 *>(filter)[i];              // (the workspace is 16-byte aligned)
    const uint32_t n_pos = text_bytes - window + 1u;                             // the caller has text_bytes >= window
    const bool aligned = (reinterpret_cast<uintptr_t>(text) & 15u) == 0;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t t0 = tile * SC_TILE;                                      // < n_pos <= 2^32 - 1
        const uint32_t left = text_bytes - t0;
        const uint32_t have = left < SC_TILE + window - 1u ? left : SC_TILE + window - 1u;   // bytes staged, <= SC_TILE_BYTES
        __syncthreads();                                                         // the tile before this one has been read
        const uint32_t whole = aligned ? have / 16u : 0u;                        // t0 is a multiple of 16
        for (uint32_t i = tid; i < whole; i += SC_THREADS)
            s_tile4[i] = reinterpret_cast<const uint4 *>(text + t0)[i];
        for (uint32_t i = whole * 16u + tid; i < have; i += SC_THREADS) s_tile[i] = text[(size_t)t0 + i];
        __syncthreads();
        const uint32_t pos_here = n_pos - t0 < SC_TILE ? n_pos - t0 : SC_TILE;
        for (uint32_t r = 0; r < SC_PER_LANE; ++r) {
            const uint32_t p = r * SC_THREADS + tid;                             // p + window <= have
            if (p >= pos_here) break;
            Hash2 hs;
            for (uint32_t j = 0; j < window; ++j) hs.add(s_tile[p + j]);
            const unsigned long long h = hs.value(flags);
            const uint32_t bit = filter_bit(h);
            if (!((s_filter[bit >> 5] >> (bit & 31u)) & 1u)) continue;
            const unsigned long long tag = tag_of(h);
            for (uint32_t s = first_slot(h, mask);; s = (s + 1u) & mask) {
                const unsigned long long e = table[s];
                if (e == SC_EMPTY) break;
                if ((e >> 24) != tag) continue;
                const uint32_t k = (uint32_t)e & 0xFFFFFFu;
                const uint8_t *key = keys + (size_t)k * window;
                uint32_t j = 0;
                while (j < window && key[j] == s_tile[p + j]) ++j;
                if (j == window) found[k] = 1;
            }
        }
    }
}

int scan_args(pgx_ctx *ctx, const void *text, uint64_t text_bytes, const void *keys, uint32_t n_keys, uint32_t window,
              uint32_t flags, const void *found) {
    PGX_REQUIRE(ctx, "NULL argument");
    PGX_REQUIRE(window >= 1 && window <= SC_MAX_WINDOW, "window must be 1..1024");
    PGX_REQUIRE(text_bytes < (1ull << 32), "text_bytes must be below 2^32");
    PGX_REQUIRE(n_keys < (1u << 24), "n_keys must be below 2^24");
    PGX_REQUIRE((flags & ~PGX_SCAN_NARROW_HASH) == 0, "unknown flags");
    PGX_REQUIRE(n_keys == 0 || (keys && found), "NULL keys or found");
    PGX_REQUIRE(text_bytes == 0 || n_keys == 0 || text, "NULL text");
    return PGX_OK;
}

// Everything on the device; `stream` is synchronised once, at the end.
int scan_run(pgx_ctx *ctx, const uint8_t *d_text, uint64_t text_bytes, const uint8_t *d_keys, uint32_t n_keys, uint32_t window,
             uint32_t flags, uint8_t *d_found, void *d_ws, size_t ws_bytes, hipStream_t stream) {
    int rc = scan_args(ctx, d_text, text_bytes, d_keys, n_keys, window, flags, d_found);
    if (rc != PGX_OK) return rc;
    if (n_keys == 0) return PGX_OK;
    const bool any_window = text_bytes >= window;
    const ScanGeom g = make_geom(n_keys);
    if (any_window) {
        PGX_REQUIRE(d_ws && ws_bytes >= g.bytes, "workspace too small (see pgx_window_scan_workspace_bytes)");
        PGX_REQUIRE(((uintptr_t)d_ws & 15u) == 0, "workspace must be 16-byte aligned");
    }
    PGX_HIP(hipMemsetAsync(d_found, 0, n_keys, stream));
    if (any_window) {
        char *p = (char *)d_ws;
        unsigned long long *table = (unsigned long long *)(p + g.off_table);
        uint32_t *filter = (uint32_t *)(p + g.off_filter);
        PGX_HIP(hipMemsetAsync(table, 0xFF, (size_t)g.slots * 8, stream));
        PGX_HIP(hipMemsetAsync(filter, 0, (size_t)SC_FILTER_WORDS * 4, stream));
        {
            ProfScope prof(ctx, "scan_build_kernel", stream);
            scan_build_kernel<<<ceil_div_u32(n_keys, SC_THREADS), SC_THREADS, 0, stream>>>(d_keys, n_keys, window, flags, table,
                                                                                          g.slots - 1u, filter);
        }
        PGX_HIP(hipGetLastError());
        const uint64_t n_pos = text_bytes - window + 1u;
        const uint32_t n_tiles = (uint32_t)((n_pos + SC_TILE - 1) / SC_TILE);
        {
            ProfScope prof(ctx, "scan_kernel", stream);
            scan_kernel<<<std::min(n_tiles, SC_MAX_GRID), SC_THREADS, 0, stream>>>(d_text, (uint32_t)text_bytes, d_keys, window,
                                                                                  flags, table, g.slots - 1u, filter, n_tiles,
                                                                                  d_found);
        }
        PGX_HIP(hipGetLastError());
    }
    PGX_HIP(hipStreamSynchronize(stream));
    return PGX_OK;
}

int scan_host(pgx_ctx *ctx, const uint8_t *text, uint64_t text_bytes, const uint8_t *keys, uint32_t n_keys, uint32_t window,
              uint32_t flags, uint8_t *out_found) {
    int rc = scan_args(ctx, text, text_bytes, keys, n_keys, window, flags, out_found);
    if (rc != PGX_OK) return rc;
    if (n_keys == 0) return PGX_OK;
    if (text_bytes < window) { memset(out_found, 0, n_keys); return PGX_OK; }     // no window: nothing to upload
    PGX_HIP(hipSetDevice(ctx->device_id));
    hipStream_t stream = ctx->stream;
    const ScanGeom g = make_geom(n_keys);
    const size_t key_bytes = (size_t)n_keys * window;
    DevBuf d_text(ctx, SC_SLOT_TEXT), d_keys(ctx, SC_SLOT_KEYS), d_found(ctx, SC_SLOT_FOUND), d_ws(ctx, SC_SLOT_WS);
    PGX_HIP(d_text.alloc((size_t)text_bytes));
    PGX_HIP(d_keys.alloc(key_bytes));
    PGX_HIP(d_found.alloc(n_keys));
    PGX_HIP(d_ws.alloc(g.bytes));
    rc = pgx_staged_h2d(ctx, d_text.p, text, (size_t)text_bytes, stream);
    if (rc != PGX_OK) return rc;
    PGX_HIP(hipMemcpyAsync(d_keys.p, keys, key_bytes, hipMemcpyHostToDevice, stream));
    rc = scan_run(ctx, d_text.as<uint8_t>(), text_bytes, d_keys.as<uint8_t>(), n_keys, window, flags, d_found.as<uint8_t>(),
                  d_ws.p, g.bytes, stream);
    if (rc != PGX_OK) return rc;
    PGX_HIP(hipMemcpyAsync(out_found, d_found.p, n_keys, hipMemcpyDeviceToHost, stream));
    PGX_HIP(hipStreamSynchronize(stream));
    return PGX_OK;
}

}  // namespace

extern "C" {

uint32_t pgx_window_scan_tile(void) { return SC_TILE; }

size_t pgx_window_scan_workspace_bytes(uint64_t text_bytes, uint32_t n_keys, uint32_t window) {
    if (!sizes_ok(text_bytes, n_keys, window)) return 0;
    return make_geom(n_keys).bytes;
}

int pgx_window_scan(pgx_ctx *ctx, const uint8_t *text, uint64_t text_bytes, const uint8_t *keys, uint32_t n_keys,
                    uint32_t window, uint32_t flags, uint8_t *out_found) {
    return guarded(__func__, [&] { return scan_host(ctx, text, text_bytes, keys, n_keys, window, flags, out_found); });
}

int pgx_window_scan_dev(pgx_ctx *ctx, const uint8_t *d_text, uint64_t text_bytes, const uint8_t *d_keys, uint32_t n_keys,
                        uint32_t window, uint32_t flags, uint8_t *d_found, void *d_workspace, size_t workspace_bytes,
                        void *stream) {
    return guarded(__func__, [&] {
        return scan_run(ctx, d_text, text_bytes, d_keys, n_keys, window, flags, d_found, d_workspace, workspace_bytes,
                        (hipStream_t)stream);
    });
}

}  // extern "C"
