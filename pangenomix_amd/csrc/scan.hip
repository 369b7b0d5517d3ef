// Exact multi-pattern matching of fixed-length keys (reference pangenome.py:1573-1647 validate_proximal_table_direct slides a
// window over every contig, one dict look-up per base): found[k] = 1 iff the `window` bytes of key k occur anywhere in the
// text. Bytes are bytes: no case folding, no alphabet; contigs and strands are the caller's business (pangenome.py joins the
// contigs with a byte no key holds and adds the reverse complements of the KEYS).
//
// A key is its `window` bytes, all of them hashed: the index (two polynomial hashes mixed to 64 bits, a 2^18-bit filter, an
// open-addressed table of tagged 64-bit entries) and the tile scan are text_index.h's, shared with pattern.hip and near.hip;
// its header comment has the layout. An entry's payload is the key's index (n_keys < 2^24). A key is reported only after its
// bytes have been compared with the text's, so the result is exact whatever the hash does -- PGX_SCAN_NARROW_HASH keeps 3
// bits of it and must give the same output.
//
// Kernels (plain launches on one stream; the only atomics are the build kernel's CAS on a slot and OR on a filter word):
//   scan_build_kernel   one lane per key: hash, then text_index::insert_entry
//   scan_kernel         text_index::for_each_tile with a halo of window - 1 bytes: a lane hashes the window at its
//                       position, tests the filter, and only on a hit walks the table; only on a tag match are the window's
//                       bytes (in the LDS tile) compared with the key's. Equal windows store found[k] = 1: every writer
//                       writes the same value. The walk goes on past a match to the next empty slot, so equal keys are all
//                       flagged. A lane without a position does nothing: here no lane waits for another.
#include "pgx_internal.h"
#include "text_index.h"

namespace {

using namespace text_index;

constexpr uint32_t SC_MAX_WINDOW = 1024;                 // the halo's maximum: 5 KiB of LDS for tile and halo
constexpr uint32_t SC_TAG_SHIFT = 24;

bool sizes_ok(uint64_t text_bytes, uint32_t n_keys, uint32_t window) {
    return window >= 1 && window <= SC_MAX_WINDOW && text_bytes < (1ull << 32) && n_keys < (1u << 24);
}

Geom scan_geom(uint32_t n_keys) { return make_geom(n_keys, 0); }

__global__ __launch_bounds__(TI_THREADS) void scan_build_kernel(const uint8_t *__restrict__ keys, uint32_t n_keys,
                                                                uint32_t window, uint32_t flags, u64 *table, uint32_t mask,
                                                                uint32_t *__restrict__ filter) {
    const uint32_t k = blockIdx.x * TI_THREADS + threadIdx.x;
    if (k >= n_keys) return;
    const u64 h = hash_bytes(keys + (size_t)k * window, window, flags & PGX_SCAN_NARROW_HASH);
    insert_entry(table, mask, filter, h, make_entry<SC_TAG_SHIFT>(h, k));
}

__global__ __launch_bounds__(TI_THREADS) void scan_kernel(const uint8_t *__restrict__ text, uint32_t text_bytes,
                                                          const uint8_t *__restrict__ keys, uint32_t window, uint32_t flags,
                                                          const u64 *__restrict__ table, uint32_t mask,
                                                          const uint32_t *__restrict__ filter, uint32_t n_tiles,
                                                          uint8_t *__restrict__ found) {
    for_each_tile<SC_MAX_WINDOW>(text, text_bytes, window, filter, n_tiles,
        [&](uint32_t, uint32_t pos_here, const uint8_t *s_tile, const uint32_t *s_filter) {
            // its own rounds: no lane waits for another here, so a lane leaves with its last position
            for (uint32_t r = 0; r < TI_TILE / TI_THREADS; ++r) {
                const uint32_t p = r * TI_THREADS + threadIdx.x;
                if (p >= pos_here) break;
                const u64 h = hash_bytes(s_tile + p, window, flags & PGX_SCAN_NARROW_HASH);
                if (!filter_has(s_filter, h)) continue;
                const u64 tag = h >> SC_TAG_SHIFT;
                for (uint32_t s = first_slot(h, mask);; s = (s + 1u) & mask) {
                    const u64 e = table[s];
                    if (e == TI_EMPTY) break;
                    if ((e >> SC_TAG_SHIFT) != tag) continue;
                    const uint32_t k = (uint32_t)e & 0xFFFFFFu;
                    const uint8_t *key = keys + (size_t)k * window;
                    uint32_t j = 0;
                    while (j < window && key[j] == s_tile[p + j]) ++j;
                    if (j == window) found[k] = 1;
                }
            }
        });
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
    const Geom g = scan_geom(n_keys);
    if (any_window) {
        PGX_REQUIRE(d_ws && ws_bytes >= g.bytes, "workspace too small (see pgx_window_scan_workspace_bytes)");
        PGX_REQUIRE(((uintptr_t)d_ws & 15u) == 0, "workspace must be 16-byte aligned");
    }
    PGX_HIP(hipMemsetAsync(d_found, 0, n_keys, stream));
    if (any_window) {
        PGX_HIP(enqueue_clear(d_ws, g, stream));
        {
            ProfScope prof(ctx, "scan_build_kernel", stream);
            scan_build_kernel<<<ceil_div_u32(n_keys, TI_THREADS), TI_THREADS, 0, stream>>>(d_keys, n_keys, window, flags,
                                                                                          g.table(d_ws), g.mask(), g.filter(d_ws));
        }
        PGX_HIP(hipGetLastError());
        const uint32_t n_tiles = tiles_of(text_bytes, window);
        {
            ProfScope prof(ctx, "scan_kernel", stream);
            scan_kernel<<<grid_of(n_tiles), TI_THREADS, 0, stream>>>(d_text, (uint32_t)text_bytes, d_keys, window, flags,
                                                                    g.table(d_ws), g.mask(), g.filter(d_ws), n_tiles, d_found);
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
    const Geom g = scan_geom(n_keys);
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

uint32_t pgx_window_scan_tile(void) { return TI_TILE; }

size_t pgx_window_scan_workspace_bytes(uint64_t text_bytes, uint32_t n_keys, uint32_t window) {
    if (!sizes_ok(text_bytes, n_keys, window)) return 0;
    return scan_geom(n_keys).bytes;
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
