// Exact look-up of whole byte strings in a set of byte strings (reference pangenome.py:1418-1546 validate_table_against_fasta
// does one SHA-256 and one dict look-up per FASTA record), and the per-genome difference of two presence bitmaps that
// closes that check. Bytes are bytes: what a string means -- a sequence, a sequence with a name behind it -- is the caller's
// business. String i of a blob is the bytes [offsets[i], offsets[i + 1]); the empty string is a string like any other.
//
// A string's 64-bit hash is the wrapping sum, over its 16-byte chunks (the last one zero-padded), of mix(chunk, chunk number),
// finished with the length: a sum has no order, so the lanes of a group add their chunks in any order and a chunk's place
// still counts. The hash only decides WHERE to look: a result is reported only after lengths and bytes have been compared,
// so it is exact whatever the hash does -- PGX_DICT_NARROW_HASH keeps 3 bits of it and must give the same output.
//   bits 0-...   the first slot probed in an open-addressed table of 64-bit entries, linear probing
//   bits 24-63   the entry's 40-bit tag; its low 24 bits are the key's index (n_keys < 2^24, so an entry is never the
//                all-ones word that marks an empty slot)
// The table has at least twice as many slots as keys, so a probe sequence always reaches an empty slot; nothing is ever
// removed, so every key whose hash equals a string's lies between that string's first slot and the next empty one.
//
// Kernels (plain launches on one stream; the only atomic is the build kernel's CAS on a slot):
//   dict_build_kernel   a group of DM_GROUP lanes hashes one key, its first lane inserts it
//   dict_match_kernel   a group of DM_GROUP lanes owns one string: hashes it, walks the probe sequence to the next empty slot,
//                       and on a tag match compares lengths, then bytes -- every lane its chunks, one vote of the group.
//                       The walk goes on past a match: the result is the smallest (DM_FIRST: a key among the keys, itself
//                       included) or the largest (DM_LAST: a query among the keys, -1 for none) index of an equal key, a
//                       minimum / maximum over a set, so it does not depend on the order the keys were inserted in.
//                       The group's first lane stores it.
//   sets_diff_kernel    one workgroup per genome: popcounts of A & ~B and B & ~A over the genome's words, pad bits masked
// Chunks are read with aligned 16-byte loads where the aligned words lie inside the blob and byte by byte at its edges, so
// nothing outside [0, offsets[n]) is read, wherever the blob starts.
#include "pgx_internal.h"
#include "string_hash.h"

namespace {

using namespace string_hash;

constexpr int DM_THREADS = 256;
constexpr uint32_t DM_STEP = DM_GROUP * DM_CHUNK;          // bytes per group and step (pgx_dict_group_bytes)
constexpr uint32_t DM_GROUPS_PER_BLOCK = DM_THREADS / DM_GROUP;
constexpr uint32_t DM_MAX_GRID = 8192;
constexpr unsigned long long DM_EMPTY = ~0ull;
constexpr int DM_FIRST = 0, DM_LAST = 1;
static_assert(64 % DM_GROUP == 0 && (DM_GROUP & (DM_GROUP - 1)) == 0, "a wave holds whole groups");

uint32_t dict_slots(uint32_t n_keys) {
    uint32_t slots = 64;
    while (slots < 2 * n_keys) slots <<= 1;                // (n_keys < 2^24: at most 2^25)
    return slots;
}

__global__ __launch_bounds__(DM_THREADS) void dict_build_kernel(const uint8_t *__restrict__ keys,
                                                                const u64 *__restrict__ key_offsets, uint32_t n_keys,
                                                                uint32_t flags, u64 *table, uint32_t mask) {
    const uint32_t sub = threadIdx.x & (DM_GROUP - 1u);
    const u64 total = key_offsets[n_keys];
    const uint32_t n_rounds = (n_keys + DM_GROUPS_PER_BLOCK - 1u) / DM_GROUPS_PER_BLOCK;
    // every lane takes the same number of rounds (a group without a key hashes the empty span and inserts nothing), so the
    // shuffles of group_hash are reached by whole waves
    for (uint32_t round = blockIdx.x; round < n_rounds; round += gridDim.x) {
        const uint32_t k = round * DM_GROUPS_PER_BLOCK + threadIdx.x / DM_GROUP;
        const bool live = k < n_keys;
        u64 begin = 0, len = 0;
        if (live) string_span(key_offsets, k, total, begin, len);
        Chunk first;
        const u64 h = group_hash(keys, total, begin, len, sub, flags, first);
        if (!live || sub != 0u) continue;
        const u64 entry = ((h >> 24) << 24) | k;
        uint32_t s = (uint32_t)h & mask;
        // `mask + 1` >= 2 * n_keys slots, of which fewer than n_keys are taken: an empty one is always met
        for (;;) {
            if (__atomic_load_n(&table[s], __ATOMIC_RELAXED) == DM_EMPTY && atomicCAS(&table[s], DM_EMPTY, entry) == DM_EMPTY)
                break;
            s = (s + 1u) & mask;
        }
    }
}

__global__ __launch_bounds__(DM_THREADS) void dict_match_kernel(const uint8_t *__restrict__ strings,
                                                                const u64 *__restrict__ offsets, uint32_t n_strings,
                                                                const uint8_t *__restrict__ keys,
                                                                const u64 *__restrict__ key_offsets, uint32_t n_keys,
                                                                uint32_t flags, const u64 *__restrict__ table, uint32_t mask,
                                                                int mode, int32_t *__restrict__ out) {
    const uint32_t sub = threadIdx.x & (DM_GROUP - 1u);
    const uint32_t lane = threadIdx.x & 63u;
    const u64 group_lanes = ((1ull << DM_GROUP) - 1ull) << (lane & ~(DM_GROUP - 1u));
    const u64 total = offsets[n_strings], key_total = key_offsets[n_keys];
    const uint32_t n_rounds = (n_strings + DM_GROUPS_PER_BLOCK - 1u) / DM_GROUPS_PER_BLOCK;
    for (uint32_t round = blockIdx.x; round < n_rounds; round += gridDim.x) {
        const uint32_t i = round * DM_GROUPS_PER_BLOCK + threadIdx.x / DM_GROUP;
        const bool live = i < n_strings;
        u64 begin = 0, len = 0;
        if (live) string_span(offsets, i, total, begin, len);
        Chunk first;
        const u64 h = group_hash(strings, total, begin, len, sub, flags, first);
        const u64 tag = h >> 24;
        const u64 n_chunks = (len + DM_CHUNK - 1) / DM_CHUNK;
        int32_t best = mode == DM_FIRST ? 0x7FFFFFFF : -1;
        // live, s, e, k and the key's span are the same on every lane of a group, so a group leaves the walk as one; the
        // vote is taken by every lane still walking, a lane that has nothing to compare voting "equal"
        bool walking = live;
        uint32_t s = (uint32_t)h & mask;
        while (walking) {
            const u64 e = table[s];
            s = (s + 1u) & mask;
            bool differs = false, candidate = false;
            uint32_t k = 0;
            if (e == DM_EMPTY) walking = false;
            else if ((e >> 24) == tag) {
                k = (uint32_t)e & 0xFFFFFFu;
                u64 kb, kl;
                string_span(key_offsets, k, key_total, kb, kl);
                candidate = kl == len;
                if (candidate) {
                    for (u64 c = sub; c < n_chunks; c += DM_GROUP) {
                        const u64 left = len - c * DM_CHUNK;
                        const uint32_t n = left < DM_CHUNK ? (uint32_t)left : DM_CHUNK;
                        const Chunk q = c == sub ? first : load_chunk(strings, total, begin + c * DM_CHUNK, n);
                        const Chunk t = load_chunk(keys, key_total, kb + c * DM_CHUNK, n);
                        differs |= (q.lo != t.lo) | (q.hi != t.hi);
                    }
                }
            }
            const u64 votes = __ballot(differs) & group_lanes;
            if (candidate && votes == 0ull) {
                const int32_t ki = (int32_t)k;
                best = mode == DM_FIRST ? (ki < best ? ki : best) : (ki > best ? ki : best);
            }
        }
        if (live && sub == 0u) out[i] = best;
    }
}

__global__ __launch_bounds__(DM_THREADS) void sets_diff_kernel(const u64 *__restrict__ a_bits, const u64 *__restrict__ b_bits,
                                                               uint32_t n_rows, uint32_t stride,
                                                               uint32_t *__restrict__ a_only, uint32_t *__restrict__ b_only) {
    __shared__ uint32_t s_part[2][DM_THREADS / 64];
    const uint32_t g = blockIdx.x, tid = threadIdx.x;
    const u64 *a = a_bits + (size_t)g * stride, *b = b_bits + (size_t)g * stride;
    const uint32_t words = (n_rows + 63u) / 64u;                       // <= stride; the rest of the stride is padding
    const u64 last_mask = (n_rows & 63u) ? (1ull << (n_rows & 63u)) - 1ull : ~0ull;
    uint32_t na = 0, nb = 0;
    for (uint32_t w = tid; w < words; w += DM_THREADS) {
        const u64 keep = w + 1u == words ? last_mask : ~0ull;          // pad bits are masked, not trusted
        const u64 x = a[w] & keep, y = b[w] & keep;
        na += (uint32_t)__popcll(x & ~y);
        nb += (uint32_t)__popcll(y & ~x);
    }
    for (int d = 32; d >= 1; d >>= 1) {
        na += (uint32_t)__shfl_xor((int)na, d, 64);
        nb += (uint32_t)__shfl_xor((int)nb, d, 64);
    }
    if ((tid & 63u) == 0u) { s_part[0][tid >> 6] = na; s_part[1][tid >> 6] = nb; }
    __syncthreads();
    if (tid == 0u) {
        uint32_t ta = 0, tb = 0;
        for (int w = 0; w < DM_THREADS / 64; ++w) { ta += s_part[0][w]; tb += s_part[1][w]; }
        a_only[g] = ta;
        b_only[g] = tb;
    }
}

// ---- launches ------------------------------------------------------------------------------------------------------------
uint32_t rounds_grid(uint32_t n_strings) {
    const uint32_t rounds = ceil_div_u32(n_strings, DM_GROUPS_PER_BLOCK);
    return rounds < DM_MAX_GRID ? rounds : DM_MAX_GRID;
}

int dict_sizes(pgx_ctx *ctx, uint32_t n_keys, uint32_t flags) {
    PGX_REQUIRE(ctx, "NULL argument");
    PGX_REQUIRE(n_keys < (1u << 24), "n_keys must be below 2^24");
    PGX_REQUIRE((flags & ~PGX_DICT_NARROW_HASH) == 0, "unknown flags");
    return PGX_OK;
}

// one int32 per query comes back and a launch takes ceil(n / 16) rounds in 32 bits
constexpr uint32_t DM_MAX_QUERIES = 1u << 31;

int dict_build(pgx_ctx *ctx, const uint8_t *d_keys, const u64 *d_key_offsets, uint32_t n_keys, uint32_t flags, u64 *d_table,
               hipStream_t stream) {
    const uint32_t slots = dict_slots(n_keys);
    PGX_HIP(hipMemsetAsync(d_table, 0xFF, (size_t)slots * 8, stream));
    {
        ProfScope prof(ctx, "dict_build_kernel", stream);
        dict_build_kernel<<<rounds_grid(n_keys), DM_THREADS, 0, stream>>>(d_keys, d_key_offsets, n_keys, flags, d_table,
                                                                         slots - 1u);
    }
    PGX_HIP(hipGetLastError());
    return PGX_OK;
}

int dict_match(pgx_ctx *ctx, const uint8_t *d_strings, const u64 *d_offsets, uint32_t n_strings, const uint8_t *d_keys,
               const u64 *d_key_offsets, uint32_t n_keys, uint32_t flags, const u64 *d_table, int mode, int32_t *d_out,
               hipStream_t stream) {
    if (n_strings == 0) return PGX_OK;
    if (n_keys == 0) {                                                       // nothing to find: -1 everywhere
        PGX_HIP(hipMemsetAsync(d_out, 0xFF, (size_t)n_strings * 4, stream));
        return PGX_OK;
    }
    {
        ProfScope prof(ctx, mode == DM_FIRST ? "dict_match_kernel(first)" : "dict_match_kernel(last)", stream);
        dict_match_kernel<<<rounds_grid(n_strings), DM_THREADS, 0, stream>>>(d_strings, d_offsets, n_strings, d_keys,
                                                                            d_key_offsets, n_keys, flags, d_table,
                                                                            dict_slots(n_keys) - 1u, mode, d_out);
    }
    PGX_HIP(hipGetLastError());
    return PGX_OK;
}

// Everything on the device; `stream` is synchronised once, at the end.
int dict_match_dev(pgx_ctx *ctx, const uint8_t *d_keys, const u64 *d_key_offsets, uint32_t n_keys, const uint8_t *d_queries,
                   const u64 *d_query_offsets, uint32_t n_queries, uint32_t flags, int32_t *d_out_first, int32_t *d_out_last,
                   void *d_ws, size_t ws_bytes, hipStream_t stream) {
    int rc = dict_sizes(ctx, n_keys, flags);
    if (rc != PGX_OK) return rc;
    PGX_REQUIRE(n_queries < DM_MAX_QUERIES, "n_queries must be below 2^31");
    PGX_REQUIRE(n_keys == 0 || (d_keys && d_key_offsets), "NULL keys or key_offsets");
    PGX_REQUIRE(n_queries == 0 || (d_queries && d_query_offsets && d_out_last), "NULL queries, query_offsets or out_last");
    if (n_keys) {
        PGX_REQUIRE(d_ws && ws_bytes >= (size_t)dict_slots(n_keys) * 8, "workspace too small (see pgx_dict_workspace_bytes)");
        PGX_REQUIRE(((uintptr_t)d_ws & 15u) == 0, "workspace must be 16-byte aligned");
        PGX_REQUIRE(((uintptr_t)d_key_offsets & 7u) == 0, "offsets must be 8-byte aligned");
    }
    PGX_REQUIRE(n_queries == 0 || ((uintptr_t)d_query_offsets & 7u) == 0, "offsets must be 8-byte aligned");
    u64 *table = (u64 *)d_ws;
    if (n_keys) {
        rc = dict_build(ctx, d_keys, d_key_offsets, n_keys, flags, table, stream);
        if (rc != PGX_OK) return rc;
        if (d_out_first) {
            rc = dict_match(ctx, d_keys, d_key_offsets, n_keys, d_keys, d_key_offsets, n_keys, flags, table, DM_FIRST,
                            d_out_first, stream);
            if (rc != PGX_OK) return rc;
        }
    }
    rc = dict_match(ctx, d_queries, d_query_offsets, n_queries, d_keys, d_key_offsets, n_keys, flags, table, DM_LAST,
                    d_out_last, stream);
    if (rc != PGX_OK) return rc;
    PGX_HIP(hipStreamSynchronize(stream));
    return PGX_OK;
}

// offsets of a host entry: n + 1 entries that never decrease, below 2^32
int host_offsets_ok(const uint64_t *offsets, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) PGX_REQUIRE(offsets[i] <= offsets[i + 1], "offsets must not decrease");
    PGX_REQUIRE(offsets[n] < (1ull << 32), "a blob must hold fewer than 2^32 bytes");
    return PGX_OK;
}

int upload_strings(pgx_ctx *ctx, DevBuf &d_blob, DevBuf &d_off, const uint8_t *blob, const uint64_t *offsets, uint32_t n) {
    const size_t bytes = (size_t)offsets[n];
    PGX_HIP(d_blob.alloc(bytes));
    PGX_HIP(d_off.alloc(((size_t)n + 1) * 8));
    if (bytes) {
        int rc = pgx_staged_h2d(ctx, d_blob.p, blob, bytes, ctx->stream);
        if (rc != PGX_OK) return rc;
    }
    PGX_HIP(hipMemcpyAsync(d_off.p, offsets, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    return PGX_OK;
}

int dict_load_host(pgx_ctx *ctx, const uint8_t *keys, const uint64_t *key_offsets, uint32_t n_keys, uint32_t flags,
                   int32_t *out_first) {
    int rc = dict_sizes(ctx, n_keys, flags);
    if (rc != PGX_OK) return rc;
    PGX_REQUIRE(key_offsets, "NULL key_offsets");
    rc = host_offsets_ok(key_offsets, n_keys);
    if (rc != PGX_OK) return rc;
    PGX_REQUIRE(key_offsets[n_keys] == 0 || keys, "NULL keys");
    PGX_HIP(hipSetDevice(ctx->device_id));
    ctx->dict_loaded = false;
    DevBuf d_keys(ctx, DM_SLOT_KEYS), d_off(ctx, DM_SLOT_KEY_OFF), d_table(ctx, DM_SLOT_TABLE), d_out(ctx, DM_SLOT_OUT);
    rc = upload_strings(ctx, d_keys, d_off, keys, key_offsets, n_keys);
    if (rc != PGX_OK) return rc;
    PGX_HIP(d_table.alloc((size_t)dict_slots(n_keys) * 8));
    if (n_keys) {
        rc = dict_build(ctx, d_keys.as<uint8_t>(), d_off.as<u64>(), n_keys, flags, d_table.as<u64>(), ctx->stream);
        if (rc != PGX_OK) return rc;
        if (out_first) {
            PGX_HIP(d_out.alloc((size_t)n_keys * 4));
            rc = dict_match(ctx, d_keys.as<uint8_t>(), d_off.as<u64>(), n_keys, d_keys.as<uint8_t>(), d_off.as<u64>(), n_keys,
                            flags, d_table.as<u64>(), DM_FIRST, d_out.as<int32_t>(), ctx->stream);
            if (rc != PGX_OK) return rc;
            PGX_HIP(hipMemcpyAsync(out_first, d_out.p, (size_t)n_keys * 4, hipMemcpyDeviceToHost, ctx->stream));
        }
    }
    PGX_HIP(hipStreamSynchronize(ctx->stream));
    ctx->dict_loaded = true;
    ctx->dict_keys = n_keys;
    ctx->dict_flags = flags;
    ctx->dict_d_keys = d_keys.p;
    ctx->dict_d_offsets = d_off.p;
    ctx->dict_d_table = d_table.p;
    return PGX_OK;
}

int dict_query_host(pgx_ctx *ctx, const uint8_t *queries, const uint64_t *query_offsets, uint32_t n_queries,
                    int32_t *out_last) {
    PGX_REQUIRE(ctx, "NULL argument");
    PGX_REQUIRE(ctx->dict_loaded, "no set of keys is loaded (pgx_dict_load)");
    PGX_REQUIRE(n_queries < DM_MAX_QUERIES, "n_queries must be below 2^31");
    PGX_REQUIRE(query_offsets, "NULL query_offsets");
    int rc = host_offsets_ok(query_offsets, n_queries);
    if (rc != PGX_OK) return rc;
    if (n_queries == 0) return PGX_OK;
    PGX_REQUIRE(out_last && (query_offsets[n_queries] == 0 || queries), "NULL queries or out_last");
    PGX_HIP(hipSetDevice(ctx->device_id));
    const uint32_t n_keys = ctx->dict_keys;
    // the loaded set: the pointers pgx_dict_load left in the context (its slots are touched by nothing else)
    const uint8_t *d_keys = static_cast<const uint8_t *>(ctx->dict_d_keys);
    const u64 *d_off = static_cast<const u64 *>(ctx->dict_d_offsets), *d_table = static_cast<const u64 *>(ctx->dict_d_table);
    DevBuf d_q(ctx, DM_SLOT_QUERIES), d_qoff(ctx, DM_SLOT_QUERY_OFF), d_out(ctx, DM_SLOT_OUT);
    rc = upload_strings(ctx, d_q, d_qoff, queries, query_offsets, n_queries);
    if (rc != PGX_OK) return rc;
    PGX_HIP(d_out.alloc((size_t)n_queries * 4));
    rc = dict_match(ctx, d_q.as<uint8_t>(), d_qoff.as<u64>(), n_queries, d_keys, d_off, n_keys, ctx->dict_flags, d_table,
                    DM_LAST, d_out.as<int32_t>(), ctx->stream);
    if (rc != PGX_OK) return rc;
    PGX_HIP(hipMemcpyAsync(out_last, d_out.p, (size_t)n_queries * 4, hipMemcpyDeviceToHost, ctx->stream));
    PGX_HIP(hipStreamSynchronize(ctx->stream));
    return PGX_OK;
}

int sets_diff_launch(pgx_ctx *ctx, const u64 *d_a, const u64 *d_b, uint32_t n_rows, uint32_t n_genomes, uint32_t *d_a_only,
                     uint32_t *d_b_only, hipStream_t stream) {
    PGX_REQUIRE(ctx, "NULL argument");
    PGX_REQUIRE(n_rows < (1u << 31) && n_genomes < (1u << 31), "n_rows and n_genomes must be below 2^31");
    if (n_genomes == 0) return PGX_OK;
    PGX_REQUIRE(d_a && d_b && d_a_only && d_b_only, "NULL argument");
    {
        ProfScope prof(ctx, "sets_diff_kernel", stream);
        sets_diff_kernel<<<n_genomes, DM_THREADS, 0, stream>>>(d_a, d_b, n_rows, pgx_bitmap_stride_words(n_rows), d_a_only,
                                                              d_b_only);
    }
    PGX_HIP(hipGetLastError());
    return PGX_OK;
}

int sets_diff_host(pgx_ctx *ctx, const int32_t *a_rows, const int32_t *a_genomes, uint64_t n_a, const int32_t *b_rows,
                   const int32_t *b_genomes, uint64_t n_b, uint32_t n_rows, uint32_t n_genomes, uint32_t *out_a_only,
                   uint32_t *out_b_only) {
    PGX_REQUIRE(ctx, "NULL argument");
    PGX_REQUIRE(n_rows < (1u << 31) && n_genomes < (1u << 31), "n_rows and n_genomes must be below 2^31");
    PGX_REQUIRE((n_a == 0 || (a_rows && a_genomes)) && (n_b == 0 || (b_rows && b_genomes)), "NULL record arrays");
    if (n_genomes == 0) return PGX_OK;
    PGX_REQUIRE(out_a_only && out_b_only, "NULL argument");
    PGX_HIP(hipSetDevice(ctx->device_id));
    DevBuf d_a(ctx, SD_SLOT_A_BITS), d_acnt(ctx, SD_SLOT_A_CNT), d_b(ctx, SD_SLOT_B_BITS), d_bcnt(ctx, SD_SLOT_B_CNT);
    DevBuf d_out(ctx, SD_SLOT_OUT);
    int rc = pgx_upload_and_build_bitmap(ctx, a_rows, a_genomes, n_a, n_rows, n_genomes, SD_SLOT_ROWS, SD_SLOT_GENOMES, d_a,
                                         d_acnt);
    if (rc == PGX_OK) rc = pgx_read_record_counters(ctx, d_acnt, nullptr);   // (an index out of range fails here)
    if (rc == PGX_OK)
        rc = pgx_upload_and_build_bitmap(ctx, b_rows, b_genomes, n_b, n_rows, n_genomes, SD_SLOT_ROWS, SD_SLOT_GENOMES, d_b,
                                         d_bcnt);
    if (rc == PGX_OK) rc = pgx_read_record_counters(ctx, d_bcnt, nullptr);
    if (rc != PGX_OK) return rc;
    PGX_HIP(d_out.alloc((size_t)n_genomes * 8));
    uint32_t *o = d_out.as<uint32_t>();
    rc = sets_diff_launch(ctx, d_a.as<u64>(), d_b.as<u64>(), n_rows, n_genomes, o, o + n_genomes, ctx->stream);
    if (rc != PGX_OK) return rc;
    PGX_HIP(hipMemcpyAsync(out_a_only, o, (size_t)n_genomes * 4, hipMemcpyDeviceToHost, ctx->stream));
    PGX_HIP(hipMemcpyAsync(out_b_only, o + n_genomes, (size_t)n_genomes * 4, hipMemcpyDeviceToHost, ctx->stream));
    PGX_HIP(hipStreamSynchronize(ctx->stream));
    return PGX_OK;
}

}  // namespace

extern "C" {

uint32_t pgx_dict_group_bytes(void) { return DM_STEP; }

size_t pgx_dict_workspace_bytes(uint64_t key_bytes, uint32_t n_keys) {
    if (key_bytes >= (1ull << 32) || n_keys >= (1u << 24)) return 0;
    return (size_t)dict_slots(n_keys) * 8;
}

int pgx_dict_load(pgx_ctx *ctx, const uint8_t *keys, const uint64_t *key_offsets, uint32_t n_keys, uint32_t flags,
                  int32_t *out_first) {
    return guarded(__func__, [&] { return dict_load_host(ctx, keys, key_offsets, n_keys, flags, out_first); });
}

int pgx_dict_query(pgx_ctx *ctx, const uint8_t *queries, const uint64_t *query_offsets, uint32_t n_queries,
                   int32_t *out_last) {
    return guarded(__func__, [&] { return dict_query_host(ctx, queries, query_offsets, n_queries, out_last); });
}

int pgx_dict_match_dev(pgx_ctx *ctx, const uint8_t *d_keys, const uint64_t *d_key_offsets, uint32_t n_keys,
                       const uint8_t *d_queries, const uint64_t *d_query_offsets, uint32_t n_queries, uint32_t flags,
                       int32_t *d_out_first, int32_t *d_out_last, void *d_workspace, size_t workspace_bytes, void *stream) {
    return guarded(__func__, [&] {
        return dict_match_dev(ctx, d_keys, (const u64 *)d_key_offsets, n_keys, d_queries, (const u64 *)d_query_offsets,
                              n_queries, flags, d_out_first, d_out_last, d_workspace, workspace_bytes, (hipStream_t)stream);
    });
}

int pgx_genome_sets_diff(pgx_ctx *ctx, const int32_t *a_rows, const int32_t *a_genomes, uint64_t n_a, const int32_t *b_rows,
                         const int32_t *b_genomes, uint64_t n_b, uint32_t n_rows, uint32_t n_genomes, uint32_t *out_a_only,
                         uint32_t *out_b_only) {
    return guarded(__func__, [&] {
        return sets_diff_host(ctx, a_rows, a_genomes, n_a, b_rows, b_genomes, n_b, n_rows, n_genomes, out_a_only, out_b_only);
    });
}

int pgx_genome_sets_diff_dev(pgx_ctx *ctx, const uint64_t *d_a_bits, const uint64_t *d_b_bits, uint32_t n_rows,
                             uint32_t n_genomes, uint32_t *d_a_only, uint32_t *d_b_only, void *stream) {
    return guarded(__func__, [&]() -> int {
        int rc = sets_diff_launch(ctx, (const u64 *)d_a_bits, (const u64 *)d_b_bits, n_rows, n_genomes, d_a_only, d_b_only,
                                  (hipStream_t)stream);
        if (rc != PGX_OK) return rc;
        PGX_HIP(hipStreamSynchronize((hipStream_t)stream));
        return PGX_OK;
    });
}

}  // extern "C"
